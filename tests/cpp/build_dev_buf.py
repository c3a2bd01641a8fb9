"""Compile tests/cpp/dev_buf_driver.cpp (DevPool and DevBuf of visma_amd/csrc/dev_buf.h: the engine's buffers and their pool
against a malloc-backed allocator that fails on demand) with -fsanitize=address,undefined.  The driver is a program of its
own: it links neither the library nor HIP and needs no GPU; the binary (tests/cpp/_build/, git-ignored) travels with the
tree like the other prebuilt drivers."""
import os
import subprocess

from build_shim import HERE, OUT, ROOT

BINS = ["dev_buf_driver"]


def build():
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, BINS[0])
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: it runs whatever else a process loads first
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "visma_amd", "csrc"),
           os.path.join(HERE, "dev_buf_driver.cpp"), "-o", out]
    subprocess.check_call(cmd)
    return [out]


if __name__ == "__main__":
    print(build())
