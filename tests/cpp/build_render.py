"""Compile tests/cpp/render_driver.cpp (feh::gpu::Renderer with the reference's members, and the resident chain volume ->
mesh -> cicp::RenderDepth -> Integrate) in both Eigen storage orders.  Needs Eigen headers at compile time only (found as
tests/cpp/build_shim.py finds them); the binaries (tests/cpp/_build/, git-ignored) travel with the tree like the other prebuilt
drivers."""
import os
import subprocess

from build_shim import HERE, OUT, ROOT, eigen_dir

BINS = ["render_driver", "render_driver_rowmajor"]


def build():
    e = eigen_dir()
    if e is None:
        return None
    os.makedirs(OUT, exist_ok=True)
    outs = []
    for name, extra in zip(BINS, ([], ["-DEIGEN_DEFAULT_TO_ROW_MAJOR"])):
        out = os.path.join(OUT, name)
        cmd = ["g++", "-std=c++11", "-O2", "-w"] + extra + [
            "-I" + os.path.join(ROOT, "include"), "-I" + e, os.path.join(HERE, "render_driver.cpp"), "-o",
            out, "-L" + os.path.join(ROOT, "visma_amd", "lib"), "-lvisma_icp",
            "-Wl,-rpath,$ORIGIN/../../../visma_amd/lib"]
        subprocess.check_call(cmd)
        outs.append(out)
    return outs


if __name__ == "__main__":
    print(build())
