"""Compile tests/cpp/colormap_solve_driver.cpp (visma_amd/csrc/colormap_solve.hpp: the host half of the non-rigid color map
optimization -- the banded assembly and solve of one camera, every camera on host threads) with
-fsanitize=address,undefined.  The driver is a program of its own: it links neither the library nor Eigen and needs no GPU;
the binary (tests/cpp/_build/, git-ignored) travels with the tree like the other prebuilt drivers."""
import os
import subprocess

from build_shim import HERE, OUT, ROOT

BINS = ["colormap_solve_driver"]


def build():
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, BINS[0])
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: it runs whatever else a process loads first
           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "visma_amd", "csrc"),
           os.path.join(HERE, "colormap_solve_driver.cpp"), "-o", out]
    subprocess.check_call(cmd)
    return [out]


if __name__ == "__main__":
    print(build())
