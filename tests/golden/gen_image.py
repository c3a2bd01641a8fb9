"""Generate tests/golden/image.npz: what the compiled reference's Image.cpp, ImageFactory.cpp, RGBDImage.cpp and
RGBDImageFactory.cpp make of the cases of tests/image_cases.py.  tests/test_image_spec.py pins the numpy specification
(tests/image_spec.py) with it, and tests/test_image.py the library with the specification.  Run once where the reference
checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there against
the reference's Core/Geometry (Image, ImageFactory, RGBDImage, RGBDImageFactory), Core/Camera/PinholeCameraIntrinsic.cpp,
Core/Utility and jsoncpp, runs it and records per case <c>:

  <c>_info        per register: width, height, channels, bytes per channel
  <c>_sha         SHA-256 of the registers' bytes and the results (tests/image_cases.py: digest)
  <c>_px<k>       register k in full (tests/image_cases.py: bits), where it has at most image_cases.FULL_BYTES bytes
  <c>_results     the float_value_at results (ok, value per step) as their f64 bits
Bits are compared as image_cases.bits gives them: every NaN as one pattern.

The flags: g++ -std=c++11 -O2 -fopenmp, WITHOUT -march=native and WITHOUT -ffast-math: x86-64's baseline has no FMA, so no
contraction enters the reference side, and SSE keeps denormals.

It asserts the properties that make each case bite (a case cannot silently stop testing anything), that the defined-domain
cases are inside the defined domain, and that the specification equals the reference bit for bit (the tests repeat that from
the fixture).  The SUN and NYU factories of the reference rewrite their depth argument: the harness hands them a copy, as
the library leaves its input alone.  Nothing compiled and no reference text is kept."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VISMA_REF", "/root/reference")
O3D = os.path.join(REF, "thirdparty", "Open3D")
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="image_")        # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_spec as S  # noqa: E402
import image_cases as cases  # noqa: E402

HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <Core/Geometry/Image.h>
#include <Core/Geometry/RGBDImage.h>
#include <Core/Camera/PinholeCameraIntrinsic.h>
using namespace open3d;
static FILE *f, *o;
static double rd() { double v; if (fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }
static std::vector<double> rvec() { std::vector<double> v((size_t)rd()); for (auto &x : v) x = rd(); return v; }
static void wimage(const Image &m)
{
    const int info[4] = {m.width_, m.height_, m.num_of_channels_, m.bytes_per_channel_};
    fwrite(info, 4, 4, o);
    if (!m.data_.empty()) fwrite(m.data_.data(), 1, m.data_.size(), o);
}
int main(int argc, char **argv)
{
    f = std::fopen(argv[1], "rb"); o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    std::vector<Image> r;
    std::vector<double> results;
    const int n_in = ri();
    for (int k = 0; k < n_in; k++) {
        Image m;
        const int w = ri(), h = ri(), ch = ri(), b = ri();
        m.PrepareImage(w, h, ch, b);
        if (!m.data_.empty() && fread(m.data_.data(), 1, m.data_.size(), f) != m.data_.size()) return 2;
        r.push_back(m);
    }
    const int nops = ri();
    for (int k = 0; k < nops; k++) {
        const int op = ri();
        switch (op) {
        case 0: { const int s = ri(), t = ri();
                  r.push_back(*CreateFloatImageFromImage(r[s], t == 0 ? Image::ColorToIntensityConversionType::Equal
                                                                      : Image::ColorToIntensityConversionType::Weighted)); break; }
        case 1: { const int s = ri(); const double a = rd(), b = rd(); r.push_back(*ConvertDepthToFloatImage(r[s], a, b)); break; }
        case 2: { const int s = ri(), b = ri();
                  r.push_back(b == 1 ? *CreateImageFromFloatImage<uint8_t>(r[s]) : *CreateImageFromFloatImage<uint16_t>(r[s])); break; }
        case 3: { const int s = ri(), t = ri(); r.push_back(*FilterImage(r[s], (Image::FilterType)t)); break; }
        case 4: { const int s = ri(); const std::vector<double> dx = rvec(), dy = rvec(); r.push_back(*FilterImage(r[s], dx, dy)); break; }
        case 5: { const int s = ri(); const std::vector<double> kk = rvec(); r.push_back(*FilterHorizontalImage(r[s], kk)); break; }
        case 6: { const int s = ri(); r.push_back(*FlipImage(r[s])); break; }
        case 7: { const int s = ri(); r.push_back(*DownsampleImage(r[s])); break; }
        case 8: { const int s = ri(), kk = ri(); r.push_back(*DilateImage(r[s], kk)); break; }
        case 9: { const int s = ri(); const double a = rd(), b = rd(); LinearTransformImage(r[s], a, b); break; }
        case 10: { const int s = ri(); const double a = rd(), b = rd(); ClipIntensityImage(r[s], a, b); break; }
        case 11: { const int s = ri(), levels = ri(), g = ri();
                   const ImagePyramid p = CreateImagePyramid(r[s], (size_t)levels, g != 0);
                   for (auto &m : p) r.push_back(*m);
                   break; }
        case 12: { const int first = ri(), count = ri(), t = ri();
                   ImagePyramid in;
                   for (int i = 0; i < count; i++) in.push_back(std::make_shared<Image>(r[first + i]));
                   const ImagePyramid p = FilterImagePyramid(in, (Image::FilterType)t);
                   for (auto &m : p) r.push_back(*m);
                   break; }
        case 13: { const double fx = rd(), fy = rd(), cx = rd(), cy = rd(); const int w = ri(), h = ri();
                   PinholeCameraIntrinsic cam(w, h, fx, fy, cx, cy);
                   r.push_back(*CreateDepthToCameraDistanceMultiplierFloatImage(cam)); break; }
        case 14: { const int s = ri(); const std::vector<double> uv = rvec();
                   std::vector<double> ok, val;
                   for (size_t i = 0; i + 1 < uv.size(); i += 2) { auto p = r[s].FloatValueAt(uv[i], uv[i + 1]); ok.push_back(p.first ? 1.0 : 0.0); val.push_back(p.second); }
                   results.insert(results.end(), ok.begin(), ok.end());
                   results.insert(results.end(), val.begin(), val.end());
                   break; }
        case 15: { const int c = ri(), d = ri(), fmt = ri(); const double a = rd(), b = rd(); const bool conv = ri() != 0;
                   const Image depth = r[d];                 // a copy: SUN and NYU rewrite it
                   std::shared_ptr<RGBDImage> p;
                   switch (fmt) {
                   case 0: p = CreateRGBDImageFromColorAndDepth(r[c], depth, a, b, conv); break;
                   case 1: p = CreateRGBDImageFromRedwoodFormat(r[c], depth, conv); break;
                   case 2: p = CreateRGBDImageFromTUMFormat(r[c], depth, conv); break;
                   case 3: p = CreateRGBDImageFromSUNFormat(r[c], depth, conv); break;
                   default: p = CreateRGBDImageFromNYUFormat(r[c], depth, conv); break;
                   }
                   r.push_back(p->color_); r.push_back(p->depth_);
                   break; }
        case 16: { const int s = ri(); r.push_back(r[s]); break; }
        default: return 3;
        }
    }
    const int n = (int)r.size();
    fwrite(&n, 4, 1, o);
    for (auto &m : r) wimage(m);
    const int nr = (int)results.size();
    fwrite(&nr, 4, 1, o);
    if (nr) fwrite(results.data(), 8, (size_t)nr, o);
    std::fclose(o);
    return 0;
}
'''


def build():
    os.makedirs(SCRATCH, exist_ok=True)
    src = os.path.join(SCRATCH, "harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(SCRATCH, "harness")
    core = os.path.join(O3D, "src", "Core")
    json = os.path.join(O3D, "3rdparty", "jsoncpp")
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"), "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D,
           "-I" + os.path.join(json, "include"), src, os.path.join(core, "Camera", "PinholeCameraIntrinsic.cpp")]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("Image", "ImageFactory", "RGBDImage", "RGBDImageFactory")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper", "IJsonConvertible")]
    cmd += [os.path.join(json, "json_" + n + ".cpp") for n in ("value", "reader", "writer")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32}


def reference(exe, inputs, program):
    """-> the reference's registers (arrays as the specification has them) and results"""
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    with open(inp, "wb") as f:
        f.write(cases.encode(inputs, program))
    subprocess.check_call([exe, inp, outp], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    raw = open(outp, "rb").read()
    at = [0]

    def take(n):
        out = raw[at[0]:at[0] + n]
        assert len(out) == n
        at[0] += n
        return out

    regs = []
    for _ in range(int(np.frombuffer(take(4), "<i4")[0])):
        w, h, ch, b = np.frombuffer(take(16), "<i4").tolist()
        if ch == 0:
            assert (w, h, b) == (0, 0, 0)
            regs.append(S.EMPTY)
            continue
        a = np.frombuffer(take(w * h * ch * b), DTYPES[b]).copy()
        regs.append(a.reshape((h, w) if ch == 1 else (h, w, ch)))
    results = np.frombuffer(take(8 * int(np.frombuffer(take(4), "<i4")[0])), "<f8").copy()
    assert at[0] == len(raw)
    return regs, results


def bite(name, regs, results):
    """the properties that make a case test something, on the REFERENCE's registers"""
    inputs, program = cases.load()[name]
    f32 = lambda a: a.dtype == np.float32
    if name.startswith("shape_"):
        w, h = [int(v) for v in name[6:].split("x")]
        assert S.info(regs[0])[:2] == (w, h) and S.info(regs[6])[:2] == (h, w) and S.info(regs[7]) == (w // 2, h // 2, 1, 4)
        assert S.is_empty(regs[10]) and S.is_empty(regs[12]) and not S.is_empty(regs[9])
        if w * h >= 36:
            assert np.isnan(regs[1]).any() and np.isinf(regs[1]).any()
    if name == "shape_65x33":
        assert len(cases.TAPS71) > 65 and not S.is_empty(regs[15]) and S.info(regs[16]) == (65, 33, 1, 4)
        # the nine weights are not dyadic, and at least one fp32 product rounds
        k = np.array(cases.TAPS9)
        assert (k.astype(np.float32).astype(np.float64) != k).all()
        a = inputs[0][np.isfinite(inputs[0])].astype(np.float64)
        exact = a[:, None] * k.astype(np.float32).astype(np.float64)[None, :]
        assert (exact.astype(np.float32).astype(np.float64) != exact).any()
    if name == "values":
        assert np.isinf(regs[4][:, 0]).all()                 # Sobel's 2 * FLT_MAX, in fp32
        assert np.isnan(regs[5][:, 1]).all()                 # ... and down equal columns inf - inf
        assert np.isinf(regs[6]).any() and np.isfinite(regs[1][0, 2]) and regs[1][0, 2] == cases.FLT_MAX
        g3 = regs[1][np.isfinite(regs[1])]
        assert ((np.abs(g3) > 0) & (np.abs(g3) < np.finfo(np.float32).tiny)).any()       # denormals survive
    if name.startswith("convert_"):
        ch = int(name[8])
        assert all(S.info(r)[2:] == (1, 4) for r in regs[1:])
        if ch == 2:
            assert not regs[1].any() and not regs[2].any()
        if ch == 3:
            assert cases.bits(regs[1]).tobytes() != cases.bits(regs[2]).tobytes()
    if name == "depth_trunc":
        assert regs[2][0, 0] == 0 and regs[2][0, 1] > 0 and regs[2][0, 1] < 3.0 and regs[3][0, 0] == 0 and regs[3][0, 1] > 0
    if name == "from_float":
        assert S.in_cast_domain(inputs[0], 1).all() and S.in_cast_domain(inputs[1], 2).all()
        assert regs[3][0, :6].tolist() == [0, 0, 1, 127, 254, 255] and regs[4][0, :4].tolist() == [0, 0, 1, 65535]
        assert S.is_empty(regs[5]) and S.is_empty(regs[6])
    if name == "rgbd":
        assert S.nyu_defined(inputs[3]).all() and ((inputs[2] & 7) != 0).all()
        assert S.is_empty(regs[-4]) and S.is_empty(regs[-3]) and S.info(regs[7]) == (6, 4, 1, 4) and S.info(regs[9]) == (6, 4, 3, 1)
        nyu = regs[7 + 2 * 8 + 1]
        assert nyu[0, 0] > 0 and nyu[0, 1] == 0 and nyu[0, 2] == 0          # 351.3 / 1092.5 m; 63.9 m is truncated; negative
    if name == "dilate_65x33":
        assert not regs[2].any() and regs[3].sum() == 3 * 255 and regs[4][1, 1] == 255 and regs[4][0, 2] == 0 and regs[4][2, 2] == 0
        assert (regs[6] == 255).all() and S.is_empty(regs[7])
    if name == "value_at":
        ok = results[:18]
        assert ok[:4].all() and not ok[4:8].any() and ok[8:15].all() and not ok[15:].any() and not results[36:].any()
    if name == "pyramid":
        assert [S.info(r)[:2] for r in regs[2:6]] == [(65, 33), (32, 16), (16, 8), (8, 4)]
        assert S.info(regs[18]) == (0, 0, 1, 4) and S.info(regs[16])[:2] == (1, 0) and len(regs) == 2 + 4 + 4 + 9 + 4 + 9
    if name == "front_end":
        assert S.info(regs[-1]) == (8, 4, 1, 1) and regs[16].max() == 255 and regs[16].min() == 0


def main():
    exe = build()
    fix = {}
    for name in cases.NAMES:
        inputs, program = cases.load()[name]
        regs, results = reference(exe, inputs, program)
        cases.same(cases.spec(name), (regs, results), name)       # the specification equals the reference
        bite(name, regs, results)
        fix[name + "_info"] = cases.infos(regs)
        fix[name + "_sha"] = cases.digest(regs, results)
        for k, r in enumerate(regs):
            if 0 < r.nbytes <= cases.FULL_BYTES:
                fix["%s_px%d" % (name, k)] = cases.bits(r)
        if len(results):
            fix[name + "_results"] = cases.bits(results)
        print("%s: %d registers, %d results" % (name, len(regs), len(results)))
    out = os.path.join(HERE, "image.npz")
    np.savez_compressed(out, **fix)
    print("image.npz: %d bytes; the specification equals the reference in every case" % os.path.getsize(out))
    if os.path.getsize(out) > 512 * 1024:
        raise SystemExit("the fixture is larger than 512 KB")


if __name__ == "__main__":
    main()
