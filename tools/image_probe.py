#!/usr/bin/env python
"""Times of the resident Image on one MI355X, for profiles/image_probe.txt, on a 640 x 480 frame of tests/tsdf_scene.py.

  (a) every operation alone on the whole frame: the conversions, the five named filters, a 9-tap and a 71-tap separable
      filter, flip, downsample, dilate(3), the in-place pair, a 4-level pyramid, float_value_at of 10,000 coordinates.  Every
      call makes a new object (an allocation and a free are part of it) and ends with the device idle, so the host clock
      around it is the call's time.  For the streaming operations the bytes the kernels must move, over that WHOLE-CALL time,
      are given as a share of the 8 TB/s peak: a lower bound of what the kernels reach, launch and wait included.
  (b) the front of the fragment pipeline per frame, two ways, alternated in one process:
        host      the caller converts uint16 depth and RGB8 colour on the CPU (numpy: depth / 1000, truncation; the gray is
                  not needed by an RGB8 volume), then TsdfVolume.integrate of the fp32 arrays (4 bytes per pixel uploaded)
        resident  Context.image of the uint16 depth (2 bytes per pixel) and of the colour, Context.rgbd(REDWOOD, no intensity
                  conversion), TsdfVolume.integrate of the two Images
      into two uniform 128^3 volumes that end in the same bytes (asserted).
  (c) the odometry front: rgbd(TUM) + rgbd_odometry of resident Images against numpy conversion + rgbd_odometry of arrays
      (the same T, asserted).
One warm-up round, then the median and the spread (min .. max) of --reps rounds (default 30), in a child process under its
own time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480
PEAK = 8.0e12


def spread(t):
    t = np.array(t[1:]) * 1e3
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def child(reps):
    import image_cases as cases
    import odometry_scene
    import tsdf_scene as scene
    from visma_amd import _lib
    frames, k = scene.frames(W, H, 1)
    depth, rgb, gray, E = frames[0]
    depth16 = np.minimum(depth * 1000.0, 65535.0).astype(np.uint16)
    ctx = _lib.Context(0)
    times = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        out = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    def drop(x):
        for i in (x if isinstance(x, (list, tuple)) else [x]):
            if i is not None:
                i.close()

    f = ctx.image(depth)
    d16 = ctx.image(depth16)
    c8 = ctx.image(rgb)
    mask = ctx.image(((gray > 0.6) * 255).astype(np.uint8))
    uv = np.random.default_rng(1).uniform(0.0, [W - 1.0, H - 1.0], (10000, 2))
    px = W * H
    ops = [("to_float of RGB8 (weighted)", lambda: c8.to_float(), 7 * px), ("depth_to_float of uint16", lambda: d16.depth_to_float(1000.0, 3.0), 6 * px),
           ("from_float to uint8", lambda: f.from_float(1), 5 * px)]
    ops += [("filter %s" % n, (lambda n=n: f.filter(n)), 16 * px) for n in _lib.IMAGE_FILTERS]
    ops += [("filter_separable 9 x 9 taps", lambda: f.filter_separable(cases.TAPS9, cases.TAPS9), 16 * px),
            ("filter_separable 71 x 71 taps", lambda: f.filter_separable(cases.TAPS71, cases.TAPS71), 16 * px),
            ("flip", lambda: f.flip(), 8 * px), ("downsample", lambda: f.downsample(), 5 * px), ("dilate(3)", lambda: mask.dilate(3), 4 * px),
            ("copy", lambda: f.copy(), 8 * px), ("pyramid of 4 levels, Gaussian", lambda: f.pyramid(4, True), 0),
            ("upload uint16 (Context.image)", lambda: ctx.image(depth16), 0), ("upload fp32 (Context.image)", lambda: ctx.image(depth), 0)]
    for r in range(reps + 1):
        for name, fn, _ in ops:
            drop(clock(name, fn))
        clock("linear_transform + clip_intensity (in place)", lambda: (f.linear_transform(1.0, 0.0), f.clip_intensity(-1e9, 1e9)))
        clock("float_value_at, 10,000 coordinates", lambda: f.float_value_at(uv))
    out = {"frame": "%d x %d" % (W, H), "reps": reps, "operations": {}}
    moved = {name: b for name, _, b in ops}
    moved["linear_transform + clip_intensity (in place)"] = 16 * px
    for name, t in times.items():
        s = spread(t)
        if moved.get(name):
            s["share_of_peak"] = moved[name] / (s["median_ms"] * 1e-3) / PEAK
        out["operations"][name] = s

    # (b) the front of the fragment pipeline
    times.clear()
    make = lambda: ctx.tsdf_uniform(4.0, 128, 0.04, _lib.TSDF_COLOR_RGB8, (-2.0, -2.0, -2.0))
    va, vb = make(), make()

    def host():
        d = depth16.astype(np.float32) / np.float32(1000.0)
        d[d >= 4.0] = 0.0
        va.integrate(d, rgb, k, E)

    def resident():
        with ctx.image(depth16) as d, ctx.image(rgb) as c:
            cc, dd = ctx.rgbd(c, d, "redwood", convert_rgb_to_intensity=False)
            vb.integrate(dd, cc, k, E)
            drop([cc, dd])

    for r in range(reps + 1):
        va.reset(); vb.reset()
        clock("host: numpy conversion + integrate of arrays", host)
        clock("resident: image + rgbd(REDWOOD) + integrate of Images", resident)
    assert [x.tobytes() for x in va.volume()] == [x.tobytes() for x in vb.volume()]
    out["fragment_front"] = {name: spread(t) for name, t in times.items()}

    # (c) the odometry front
    times.clear()
    sg, sd, tg, td, ko = odometry_scene.frames(W, H)
    to8 = lambda g: np.clip(g * 255.0, 0, 255).astype(np.uint8)
    to16 = lambda d: np.minimum(d * 5000.0, 65535.0).astype(np.uint16)
    raw = [to8(sg), to16(sd), to8(tg), to16(td)]
    option = _lib.odometry_option(iterations=(2, 2, 2))
    results = {}

    def host_odo():
        g = [raw[i].astype(np.float32) / np.float32(255.0) for i in (0, 2)]
        d = [raw[i].astype(np.float32) / np.float32(5000.0) for i in (1, 3)]
        for x in d:
            x[x >= 4.0] = 0.0
        results["host"] = ctx.rgbd_odometry(g[0], d[0], g[1], d[1], ko, option=option).T

    def resident_odo():
        imgs = [ctx.image(a) for a in raw]
        s = ctx.rgbd(imgs[0], imgs[1], "tum")
        t = ctx.rgbd(imgs[2], imgs[3], "tum")
        results["resident"] = ctx.rgbd_odometry(s[0], s[1], t[0], t[1], ko, option=option).T
        drop(imgs + list(s) + list(t))

    for r in range(reps + 1):
        clock("host: numpy conversion + rgbd_odometry of arrays", host_odo)
        clock("resident: image + rgbd(TUM) + rgbd_odometry of Images", resident_odo)
    assert results["host"].tobytes() == results["resident"].tobytes()
    out["odometry_front"] = {name: spread(t) for name, t in times.items()}
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.child:
        child(args.reps)
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], capture_output=True, text=True,
                       timeout=args.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        raise SystemExit("the probe's child ended with %d" % p.returncode)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print("resident Image, %s, median (min .. max) of %d rounds after one warm-up" % (out["frame"], out["reps"]))
    for title, key in (("(a) operations", "operations"), ("(b) fragment front, per frame", "fragment_front"), ("(c) odometry front, per pair", "odometry_front")):
        print(title)
        for name, s in out[key].items():
            share = "   %.2f %% of peak (whole call)" % (100.0 * s["share_of_peak"]) if "share_of_peak" in s else ""
            print("  %-58s %8.3f ms (%.3f .. %.3f)%s" % (name, s["median_ms"], s["min_ms"], s["max_ms"], share))


if __name__ == "__main__":
    main()
