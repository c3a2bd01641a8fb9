"""Compile tests/cpp/tsdf_units_driver.cpp (expand_touched_boxes of visma_amd/csrc/tsdf_units.h, the host half of a
scalable TSDF volume's touched units) with -fsanitize=address,undefined.  The driver is a program of its own: it links
neither the library nor Eigen and needs no GPU; the binary (tests/cpp/_build/, git-ignored) travels with the tree like the
other prebuilt drivers."""
import os
import subprocess

from build_shim import HERE, OUT, ROOT

BINS = ["tsdf_units_driver"]


def build():
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, BINS[0])
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: it runs whatever else a process loads first
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "visma_amd", "csrc"),
           os.path.join(HERE, "tsdf_units_driver.cpp"), "-o", out]
    subprocess.check_call(cmd)
    return [out]


if __name__ == "__main__":
    print(build())
