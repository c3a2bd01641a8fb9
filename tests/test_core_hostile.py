"""The registration core on clouds with rows that are not finite (include/visma_icp.h, "Points that are not finite").

THE RULE (DELETE AND REMAP).  A source point whose transformed position is not finite has no pair; a target point with a
coordinate that is not finite is nobody's partner; every other query gets the partner, the d2 bits and the tie-break
(lowest original index) it gets on the clouds with those rows deleted, indices in the caller's order -- in every search
kernel and every nn_mode; K, the kept pairs and the 38 statistics are those of the deleted clouds; a loop over such
clouds ends and returns the pose of the loop over the deleted clouds.

THE REFERENCE is `reference_pass` below: a plain numpy f64 brute force over the fp32-rounded finite rows of both clouds
(transform with the fp32 T as oracle.k_nn_pass does -- or with the f64 T for the exact search, which transforms in
f64 --, acceptance strictly d2 < (float)(r^2), ties to the lowest index, indices mapped back).  It only skips target
points farther than the radius from a chunk of queries along x, which cannot be partners.  Indices must EQUAL it; the d2
of the fp32 kernels must be bit-equal to oracle.k_nn_pass(grid=False) on the hostile clouds as given (that call runs on
the CPU), the d2 of the exact search within one fp32 ulp of the rounded f64 value; the statistics within 1e-9 relative
of oracle.k_reduce_stats on the DELETED clouds (test_nn_bit_exact's bar); the same clouds twice give bit-identical
statistics (no floating-point atomics).

THE CONDITION (asserted on the CPU, before any GPU result is looked at): on every case with finite rows left the
reference alone finds K >= 0.9 x (finite source rows) at pass 0 and K > 0 in every pass.  Expected neighbours per query:
M (4099 / 20011 in the cube [-1, 1]^3, r = 0.075) 20011 / 8 x 4.19 r^3 = 4.4; S (257 / 513, r = 0.5) 33; L (70000 / 3000
in [-0.5, 0.5]^3 -- _clouds(spread = 0.5): in the unit-edge cube the same count gives 1.6 and 21 % of the queries
none --, r = 0.1) 12.6.  The 0.075 of (5000, 20000) is therefore justified at nt = 20011 by this condition itself.

The GPU body is tools/core_hostile_probe.py, one child process per search policy (the policies are chosen by environment
variables read when a context is created); it returns arrays and judges nothing."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from visma_amd import synth
from test_gpu_kernels import _clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "core_hostile_probe.py")

# ns, nt, radius, spread of _clouds
SHAPES = {"M": (4099, 20011, 0.075, 1.0),      # several workgroups, a ragged tail, a grid of >= 512 cells, ring tables when forced
          "S": (257, 513, 0.5, 1.0),           # just past the tile / chunk borders, a degenerate grid
          "L": (70000, 3000, 0.1, 0.5)}        # the brute kernel's eight-points-per-thread path
MOTIONS = [None, 0.02, 0.0, 3.0, 0.01]         # in radii: keep a partner, lose it, get it back, meet the certificate

QNAN, NNAN, PINF, NINF = 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000
CYCLE = ("nan1", "nan3", "nneg", "pinf", "ninf", "mixed")


def _poke(a, rows, kind):
    """Hostile rows from bit patterns; a row keeps its other coordinates."""
    u = a.view(np.uint32)
    rows = np.asarray(rows, np.int64)
    ax = rows % 3
    if kind == "nan1":
        u[rows, ax] = QNAN
    elif kind == "nan3":
        u[rows] = QNAN
    elif kind == "nneg":                                   # a NaN with the sign bit set
        u[rows, ax] = NNAN
    elif kind == "pinf":
        u[rows, ax] = PINF
    elif kind == "ninf":
        u[rows, ax] = NINF
    elif kind == "pminf":                                  # +inf and -inf in rows of the SAME axis
        u[rows, 0] = np.where(np.arange(len(rows)) % 2 == 0, PINF, NINF).astype(np.uint32)
    elif kind == "mixed":                                  # inf and NaN in one row
        u[rows, ax] = PINF
        u[rows, (ax + 1) % 3] = QNAN
    elif kind == "pinf0":                                  # +inf in coordinate 0 of BOTH clouds: the difference is NaN
        u[rows, 0] = PINF
    elif kind == "big":                                    # finite: d2 overflows fp32, never a pair; the grid grows coarse
        a[rows, 0] = np.float32(1e30)
    elif kind == "cycle":
        for k, name in enumerate(CYCLE):
            _poke(a, rows[k::len(CYCLE)], name)
    else:
        raise ValueError(kind)


def _rows(n, place, rng):
    if place == "ends":
        return [0, n - 1]
    if place == "r6364":
        return [63, 64]
    if place == "wave":                                    # 64 rows aligned to a wave: a whole wave without a live query
        return np.arange(128, 192)
    if place == "blk256":
        return np.arange(256, 512) if n >= 512 else np.arange(0, 256)
    if place == "scat":                                    # 1 %
        return rng.choice(n, max(n // 100, 2), replace=False)
    if place == "row7":
        return [7]
    if place == "all":
        return np.arange(n)
    raise ValueError(place)


# name, shape, hostile rows of the source, of the target: (kind, placement)
CASES = [
    ("M-src-nan", "M", [("nan1", "ends"), ("nan3", "r6364"), ("nneg", "wave")], []),
    ("M-src-inf", "M", [("pinf", "blk256"), ("ninf", "ends"), ("mixed", "scat")], []),
    ("M-tgt-nan", "M", [], [("nan1", "scat"), ("nneg", "r6364"), ("nan3", "wave")]),
    ("M-tgt-pinf", "M", [], [("pinf", "ends")]),
    ("M-tgt-ninf", "M", [], [("ninf", "wave"), ("ninf", "r6364")]),
    ("M-tgt-pminf", "M", [], [("pminf", "blk256")]),
    ("M-tgt-mixed", "M", [], [("mixed", "scat"), ("pinf", "ends")]),
    ("M-both-inf", "M", [("pinf0", "scat"), ("nan1", "ends")], [("pinf0", "scat"), ("ninf", "r6364")]),
    ("M-tgt-big", "M", [("nan3", "wave")], [("big", "row7")]),
    ("M-tgt-all", "M", [], [("cycle", "all")]),
    ("M-src-all", "M", [("cycle", "all")], []),
    ("S-src", "S", [("nan3", "ends"), ("pinf", "r6364"), ("nneg", "wave")], []),
    ("S-tgt-pinf", "S", [], [("pinf", "ends")]),
    ("S-tgt-ninf", "S", [], [("ninf", "scat"), ("nan1", "r6364")]),
    ("S-both", "S", [("mixed", "wave"), ("pinf0", "ends")], [("pinf0", "ends"), ("pminf", "wave")]),
    ("S-tgt-big", "S", [("nan1", "scat")], [("big", "row7"), ("ninf", "ends")]),
    ("S-tgt-all", "S", [], [("cycle", "all")]),
    ("L-both", "L", [("nan1", "scat"), ("pinf", "blk256")], [("pinf", "ends"), ("nan3", "r6364")]),
]
CASE = {c[0]: c for c in CASES}
SMALL = [c[0] for c in CASES if c[1] != "L"]
SEED = {"S-src": 1, "S-tgt-big": 1}          # a case that misses THE CONDITION gets another seed here


@functools.lru_cache(maxsize=None)
def make_case(name):
    _, shape, hs, ht = CASE[name]
    ns, nt, r, spread = SHAPES[shape]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + SEED.get(name, 0))
    src, tgt = _clouds(rng, ns, nt, spread)
    T = synth.make_T(synth.rot_y(rng.uniform(-0.02, 0.02)), rng.standard_normal(3) * r * 0.25)
    Ts = [T]
    for m in MOTIONS[1:]:                                  # (as tools/fuzz_warm_vs_serial.py moves its clouds)
        T = synth.make_T(synth.rot_y(rng.uniform(-1, 1) * min(m, 1.0) * 0.05), rng.standard_normal(3) * r * m) @ T
        Ts.append(T)
    for a, spec in ((src, hs), (tgt, ht)):
        for kind, place in spec:
            _poke(a, _rows(len(a), place, rng), kind)
    for a in (src, tgt):
        a.setflags(write=False)
    return {"name": name, "src": src, "tgt": tgt, "r": r, "Ts": np.stack(Ts),
            "sk": np.isfinite(src).all(1), "tk": np.isfinite(tgt).all(1)}


def transform_f32(s, T):
    """oracle.k_nn_pass's transform: p = fmaf(r0, sx, fmaf(r1, sy, fmaf(r2, sz, t))) in fp32, row by row (the product of
    two fp32 values is exact in f64; the sum is rounded once more on the way to fp32)."""
    T32 = np.asarray(T, np.float64)[:3, :].astype(np.float32).astype(np.float64)
    s = s.astype(np.float64)
    p = np.empty((len(s), 3), np.float32)
    for a in range(3):
        acc = (T32[a, 2] * s[:, 2] + T32[a, 3]).astype(np.float32).astype(np.float64)
        acc = (T32[a, 1] * s[:, 1] + acc).astype(np.float32).astype(np.float64)
        p[:, a] = (T32[a, 0] * s[:, 0] + acc).astype(np.float32)
    return p.astype(np.float64)


def transform_f64(s, T):
    """the exact search's: the reference's f64 transform of the (fp32-valued) source"""
    T = np.asarray(T, np.float64)
    s = s.astype(np.float64)
    return np.stack([T[a, 0] * s[:, 0] + T[a, 1] * s[:, 1] + T[a, 2] * s[:, 2] + T[a, 3] for a in range(3)], 1)


def brute_force(p, t, r2):
    """nearest t (f64 ((dx^2 + dy^2) + dz^2), strictly below r2, lowest index on a tie) of every p -> index or -1, d2 or inf"""
    jbest = np.full(len(p), -1, np.int64)
    dbest = np.full(len(p), np.inf)
    if len(p) == 0 or len(t) == 0:
        return jbest, dbest
    ot = np.argsort(t[:, 0], kind="stable")
    ts, tx = t[ot], t[ot, 0]
    op = np.argsort(p[:, 0], kind="stable")
    R = np.sqrt(r2) * (1.0 + 1e-6)                         # |dx| > R: d2 >= dx^2 > r2, never accepted
    for c in range(0, len(p), 256):
        rows = op[c:c + 256]
        pc = p[rows]
        lo = np.searchsorted(tx, pc[:, 0].min() - R, "left")
        hi = np.searchsorted(tx, pc[:, 0].max() + R, "right")
        if hi <= lo:
            continue
        cand, oj = ts[lo:hi], ot[lo:hi]
        d = (cand[None, :, 0] - pc[:, None, 0]) ** 2
        d += (cand[None, :, 1] - pc[:, None, 1]) ** 2
        d += (cand[None, :, 2] - pc[:, None, 2]) ** 2
        m = d.min(axis=1)
        j = np.where(d == m[:, None], oj[None, :], np.iinfo(np.int64).max).min(axis=1)
        ok = m < r2
        jbest[rows] = np.where(ok, j, -1)
        dbest[rows] = np.where(ok, m, np.inf)
    return jbest, dbest


def reference_pass(src, tgt, T, r, xform="f32"):
    """THE RULE on (src, tgt): delete the rows that are not finite, brute force, map the indices back.
    -> idx (caller's order, -1: no pair), d2 (f64, inf: no pair), idx_del (the same pairs in the deleted clouds' numbering)"""
    sk, tk = np.isfinite(src).all(1), np.isfinite(tgt).all(1)
    p = (transform_f32 if xform == "f32" else transform_f64)(src[sk], T)
    pk = np.isfinite(p).all(1)                             # (a transformed position that is not finite has no pair)
    r2 = float(np.float32(r * r))
    j, d = brute_force(p[pk], tgt[tk].astype(np.float64), r2)
    jd = np.full(int(sk.sum()), -1, np.int64)
    dd = np.full(int(sk.sum()), np.inf)
    jd[pk], dd[pk] = j, d
    back = np.flatnonzero(tk)
    idx = np.full(len(src), -1, np.int32)
    d2 = np.full(len(src), np.inf)
    idx[sk] = np.where(jd >= 0, back[np.maximum(jd, 0)] if len(back) else -1, -1)
    d2[sk] = dd
    return idx, d2, jd.astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(name, xform="f32"):
    """the five passes of a case; computed once, shared by every test that needs it, never changed"""
    c = make_case(name)
    out = []
    for T in c["Ts"]:
        idx, d2, idx_del = reference_pass(c["src"], c["tgt"], T, c["r"], xform)
        for a in (idx, d2, idx_del):
            a.setflags(write=False)
        out.append((idx, d2, idx_del))
    return out


def check_condition(name, xform="f32"):
    """THE CONDITION, on the reference alone"""
    c, ref = make_case(name), reference(name, xform)
    finite_src, finite_tgt = int(c["sk"].sum()), int(c["tk"].sum())
    ks = [int((idx >= 0).sum()) for idx, _, _ in ref]
    if finite_src == 0 or finite_tgt == 0:
        assert ks == [0] * len(ks), (name, ks)
        return ks
    assert ks[0] >= 0.9 * finite_src, (name, ks, finite_src)
    assert min(ks) > 0, (name, ks)
    return ks


def deleted_stats(oracle, c, idx_del, T):
    s, t = c["src"][c["sk"]], c["tgt"][c["tk"]]
    if len(s) == 0 or len(t) == 0 or not (idx_del >= 0).any():
        return np.zeros(38)
    return oracle.k_reduce_stats(s, t, idx_del, np.asarray(T, np.float64)[:3, :])


def stats_close(st, want):
    """test_nn_bit_exact's bar"""
    return float(np.max(np.abs(st - want) / np.maximum(np.abs(want), 1.0))) < 1e-9


# ---------------------------------------------------------------------------
# CPU: the rule, the reference and the remapping, without a GPU
# ---------------------------------------------------------------------------
def test_the_cases_hold_every_row_kind_and_placement():
    kinds, places = set(), set()
    for _, _, hs, ht in CASES:
        for kind, place in hs + ht:
            kinds.add(kind)
            places.add(place)
    assert kinds == {"nan1", "nan3", "nneg", "pinf", "ninf", "pminf", "mixed", "pinf0", "big", "cycle"}
    assert places == {"ends", "r6364", "wave", "blk256", "scat", "row7", "all"}
    c = make_case("M-tgt-pminf")
    x = c["tgt"][256:512, 0]
    assert np.all(np.isposinf(x[0::2])) and np.all(np.isneginf(x[1::2]))
    c = make_case("M-src-nan")
    assert c["src"].view(np.uint32)[130, 130 % 3] == NNAN and not c["sk"][128:192].any() and c["sk"][192]
    assert np.isnan(c["src"][63]).all() and not c["sk"][[0, 63, 64, 4098]].any()
    c = make_case("M-both-inf")
    assert np.isposinf(c["src"][~c["sk"], 0]).sum() >= 38 and np.isposinf(c["tgt"][~c["tk"], 0]).sum() >= 198
    c = make_case("M-tgt-big")
    assert c["tgt"][7, 0] == np.float32(1e30) and c["tk"].all()
    assert not make_case("M-tgt-all")["tk"].any() and not make_case("M-src-all")["sk"].any()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_condition_and_rule_on_the_cpu(oracle, name):
    """THE CONDITION; and oracle.k_nn_pass(grid=False) -- `d < best` is false for NaN and inf -- implements THE RULE: on the
    hostile clouds as given it returns the reference's indices, and the d2 bits it returns on the deleted clouds."""
    c = make_case(name)
    check_condition(name)
    if c["name"].startswith("L"):
        passes = [0, 3]                                    # (70000 x 3000 on one CPU thread: two of the five passes)
    else:
        passes = range(len(MOTIONS))
    s_del, t_del = c["src"][c["sk"]], c["tgt"][c["tk"]]
    for p in passes:
        T = c["Ts"][p]
        idx, d2, idx_del = reference(name)[p]
        T32, r2f = T[:3, :].astype(np.float32), np.float32(c["r"] * c["r"])
        k, oidx, od2 = oracle.k_nn_pass(c["src"], c["tgt"], T32, r2f, grid=False)
        assert np.array_equal(oidx, idx), (name, p, np.flatnonzero(oidx != idx)[:5])
        assert k == int((idx >= 0).sum())
        assert not (oidx[~c["sk"]] >= 0).any() and not np.isin(oidx, np.flatnonzero(~c["tk"])).any()
        if len(s_del) and len(t_del):
            kd, didx, dd2 = oracle.k_nn_pass(s_del, t_del, T32, r2f, grid=False)
            assert kd == k and np.array_equal(didx, idx_del)
            assert np.array_equal(od2[c["sk"]].view(np.uint32), dd2.view(np.uint32))
        # the f64 distances of the reference and the fp32 ones of the specification agree to fp32 rounding
        m = idx >= 0
        assert np.all(np.abs(od2[m] - d2[m]) <= 4e-7 * d2[m] + 1e-12)


@pytest.mark.parametrize("name", ["S-src", "S-tgt-ninf", "S-both", "S-tgt-all", "M-tgt-pminf", "M-src-all"])
def test_the_host_driver_on_the_oracle_engine(lib, oracle, name):
    """The product's host driver over the oracle engine: per-pass API and a 10-iteration loop on the hostile clouds
    against the same on the deleted clouds -- K, the statistics, the pose, and the indices after remapping."""
    from oracle_engine import OracleEngine
    c = make_case(name)
    got = {}
    for tag, (s, t) in (("hostile", (c["src"], c["tgt"])), ("deleted", (c["src"][c["sk"]], c["tgt"][c["tk"]]))):
        eng = OracleEngine(oracle, grid=False)
        ctx = eng.context()
        ctx.set_target(t)
        ctx.set_source(s)
        per = []
        for T in c["Ts"]:
            ctx.nn_pass(T, c["r"])
            st = ctx.reduce()
            per.append((ctx.correspondence_index(), st))
        res = ctx.run(c["Ts"][0], c["r"], 10, 0.0, 0.0)
        got[tag] = (per, res, ctx.correspondence_index())
        ctx.close()
    back = np.flatnonzero(c["tk"])
    for p, ((hi, hst), (di, dst)) in enumerate(zip(got["hostile"][0], got["deleted"][0])):
        assert np.array_equal(hi, reference(name)[p][0]), (name, p)
        assert np.array_equal(hi[c["sk"]], np.where(di >= 0, back[np.maximum(di, 0)] if len(back) else -1, -1))
        assert not (hi[~c["sk"]] >= 0).any()
        assert hst[0] == dst[0] and stats_close(hst, dst), (name, p)
    h, d = got["hostile"][1], got["deleted"][1]
    assert h.num_correspondences == d.num_correspondences and h.iterations == d.iterations == 10
    assert np.all(np.isfinite(h.transformation_)) and synth.rel_frobenius(h.transformation_, d.transformation_) < 1e-9
    if not c["tk"].any() or not c["sk"].any():
        assert h.num_correspondences == 0 and synth.rel_frobenius(h.transformation_, c["Ts"][0]) < 1e-12   # identity updates


# ---------------------------------------------------------------------------
# GPU: one child process per search policy
# ---------------------------------------------------------------------------
def run_probe(tmp_path, args, arrays, env=None, timeout=240):
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **arrays)
    e = dict(os.environ)
    for k in ("VISMA_ICP_COOP", "VISMA_ICP_GRID_LANES", "VISMA_ICP_CHECK_BOX"):
        e.pop(k, None)
    e.update(env or {})
    # (every child under a time limit of its own)
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, PROBE] + args + [fin, fout], capture_output=True,
                       text=True, timeout=timeout + 30, cwd=ROOT, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return dict(np.load(fout))


def case_arrays(names):
    arrays = {"names": np.array(names)}
    for i, n in enumerate(names):
        c = make_case(n)
        arrays.update({"%d_src" % i: c["src"], "%d_tgt" % i: c["tgt"], "%d_Ts" % i: c["Ts"], "%d_r" % i: np.array(c["r"])})
    return arrays


def check_search(oracle, names, out, exact, kernels_allowed, kernels_required):
    """every pass of every case of one child against the reference, the oracle and itself"""
    xform = "f64" if exact else "f32"
    seen = set()
    for i, name in enumerate(names):
        c, ref = make_case(name), reference(name, xform)
        for p, T in enumerate(c["Ts"]):
            idx, d2, idx_del = ref[p]
            key = "%d_%d_0_" % (i, p)
            gidx, gd2, gst, kern = out[key + "idx"], out[key + "d2"], out[key + "st"], str(out[key + "kern"])
            seen.add(kern)
            assert kern in kernels_allowed, (name, p, kern)
            bad = np.flatnonzero(gidx != idx)
            K = int((idx >= 0).sum())
            print("%s pass %d kernel %s: K = %d (reference %d), %d indices differ" % (name, p, kern, int((gidx >= 0).sum()), K, len(bad)))
            assert len(bad) == 0, (name, p, kern, bad[:8], gidx[bad[:8]], idx[bad[:8]])
            assert len(gd2) == K == int(round(gst[0]))
            m = idx >= 0
            if exact:
                want = d2[m].astype(np.float32)
                assert np.all(np.abs(gd2 - want) <= np.spacing(want)), (name, p)
            else:
                _, oidx, od2 = oracle.k_nn_pass(c["src"], c["tgt"], T[:3, :].astype(np.float32), np.float32(c["r"] * c["r"]), grid=False)
                assert np.array_equal(gd2.view(np.uint32), od2[m].view(np.uint32)), (name, p)
            want = deleted_stats(oracle, c, idx_del, T)
            assert np.all(np.isfinite(gst)) and stats_close(gst, want), (name, p, float(np.max(np.abs(gst - want) / np.maximum(np.abs(want), 1.0))))
            # determinism: the same clouds again, bit for bit
            again = "%d_%d_1_" % (i, p)
            assert out[again + "st"].tobytes() == gst.tobytes() and np.array_equal(out[again + "idx"], gidx), (name, p)
            assert out[again + "d2"].tobytes() == gd2.tobytes()
    assert kernels_required <= seen, (kernels_required, seen)


# kernel policy of the probe -> (environment, exact search?, kernels a pass may report, kernels that must be reported)
POLICIES = {
    "brute": ({}, False, {"brute"}, {"brute"}),
    "serial": ({}, False, {"serial"}, {"serial"}),
    "warm": ({}, True, {"serial", "warm"}, {"serial", "warm"}),
    "ring": ({}, True, {"serial", "warm", "ring"}, {"ring"}),
    "exact": ({}, True, {"brute", "serial", "warm", "ring"}, {"warm"}),
    "auto": ({}, False, {"brute", "serial"}, {"brute", "serial"}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["brute", "serial", "warm", "ring", "exact", "auto"])
def test_every_search_kernel_follows_the_rule(lib, oracle, tmp_path, kernel):
    """brute force, lane-serial grid, warm cooperative search (one launch per pass), ring search, the exact search under
    NN_AUTO, and NN_AUTO over the fp32 kernels (the same answer as both forced modes: all three equal the reference)."""
    env, exact, allowed, required = POLICIES[kernel]
    names = SMALL + (["L-both"] if kernel in ("brute", "auto") else [])
    for n in names:
        check_condition(n, "f64" if exact else "f32")
    out = run_probe(tmp_path, ["search", kernel, "f32"], case_arrays(names), env)
    check_search(oracle, names, out, exact, allowed, required)


UPLOAD_CASES = ["M-src-inf", "M-tgt-ninf", "S-both", "S-tgt-all"]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["brute", "serial"])
def test_device_pointer_uploads_follow_the_rule(lib, oracle, tmp_path, kernel):
    """set_target_device / set_source_device from memory the library did not allocate (a torch tensor where torch sees the
    GPU in a process that also holds the library's runtime, else a plain hipMalloc; printed): no staging pass sees the points"""
    for n in UPLOAD_CASES:
        check_condition(n)
    out = run_probe(tmp_path, ["search", kernel, "device"], case_arrays(UPLOAD_CASES))
    print("device memory from", str(out["device_via"]))
    check_search(oracle, UPLOAD_CASES, out, False, {kernel}, {kernel})


@pytest.mark.gpu
@pytest.mark.parametrize("check_box", [False, True])
def test_f64_upload_rule_6_and_the_staging_box(lib, oracle, tmp_path, check_box):
    """visma_icp_set_clouds_f64 centres both clouds on the target's centroid: a TARGET coordinate that is not finite makes
    the centre non-finite and K = 0 (the documented outcome); a SOURCE row that is not finite follows the rule -- the hostile
    source against the same call with its rows deleted (the centre depends on the target alone).  With
    VISMA_ICP_CHECK_BOX=1 the staging pass's box and the device's must agree wherever the staging pass supplies one."""
    names = ["M-src-nan", "M-src-inf", "S-src", "M-tgt-pinf", "M-tgt-nan", "S-tgt-ninf"]
    arrays = case_arrays(names)
    dele = []
    for n in names[:3]:                                    # the same sources with their hostile rows deleted
        c = make_case(n)
        check_condition(n)
        i = len(names) + len(dele)
        arrays.update({"%d_src" % i: c["src"][c["sk"]], "%d_tgt" % i: c["tgt"], "%d_Ts" % i: c["Ts"], "%d_r" % i: np.array(c["r"])})
        dele.append(n + "/deleted")
    arrays["names"] = np.array(names + dele)
    out = run_probe(tmp_path, ["search", "warm", "f64"], arrays, {"VISMA_ICP_CHECK_BOX": "1"} if check_box else None)
    for i, n in enumerate(names[:3]):
        c, j = make_case(n), len(names) + i
        for p in range(len(MOTIONS)):
            h, d = "%d_%d_0_" % (i, p), "%d_%d_0_" % (j, p)
            assert np.array_equal(out[h + "idx"][c["sk"]], out[d + "idx"]) and not (out[h + "idx"][~c["sk"]] >= 0).any(), (n, p)
            assert out[h + "d2"].tobytes() == out[d + "d2"].tobytes(), (n, p)
            assert out[h + "st"][0] == out[d + "st"][0] and stats_close(out[h + "st"], out[d + "st"]), (n, p)
            # (the centred clouds are another rounding of the same points: all but a few pairs at the radius are the reference's)
            assert abs(int(out[h + "st"][0]) - int((reference(n)[p][0] >= 0).sum())) <= 2
    for i, n in enumerate(names[3:], 3):
        for p in range(len(MOTIONS)):
            k = "%d_%d_0_" % (i, p)
            assert not (out[k + "idx"] >= 0).any() and len(out[k + "d2"]) == 0 and np.all(out[k + "st"] == 0.0), (n, p)


def deleted_clouds(c):
    return c["src"][c["sk"]], c["tgt"][c["tk"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["M-both-inf", "M-tgt-pminf"])
def test_every_loop_returns_the_pose_of_the_deleted_clouds(lib, tmp_path, name):
    """run, iterate, the device loop, the persistent loop (finite timeout), run_yaw_sweep(4) and run_batch of three with a
    hostile source in the middle, 10 iterations each: the poses of the deleted clouds to 1e-9, equal K; the two clean batch
    problems bit-identical to the batch without the hostile one."""
    check_condition(name)
    c = make_case(name)
    s_del, t_del = deleted_clouds(c)
    rng = np.random.default_rng(5)
    bA = _clouds(rng, 1500, 6000)
    bC = _clouds(rng, 2100, 7001)
    bB_tgt = np.array(c["tgt"][c["tk"]])                  # (a batch centres on the target: its target is clean)
    out = run_probe(tmp_path, ["loops"], {
        "r": np.array(c["r"]), "T0": c["Ts"][0], "hostile_src": c["src"], "hostile_tgt": c["tgt"], "deleted_src": s_del,
        "deleted_tgt": t_del, "bA_src": bA[0], "bA_tgt": bA[1], "bC_src": bC[0], "bC_tgt": bC[1], "bB_tgt": bB_tgt})
    back = np.flatnonzero(c["tk"])
    for loop in ("run", "iterate", "persist", "device"):
        h, d = out["hostile_" + loop], out["deleted_" + loop]
        print(name, loop, "K", h[16], d[16], "pose difference %.3e" % synth.rel_frobenius(h[:16].reshape(4, 4), d[:16].reshape(4, 4)))
        assert np.all(np.isfinite(h)) and h[16] == d[16] > 0 and h[19] == d[19] == 10, (loop, h[16:], d[16:])
        assert synth.rel_frobenius(h[:16].reshape(4, 4), d[:16].reshape(4, 4)) < 1e-9, loop
        if loop != "iterate":
            hi, di = out["hostile_%s_idx" % loop], out["deleted_%s_idx" % loop]
            assert np.array_equal(hi[c["sk"]], np.where(di >= 0, back[np.maximum(di, 0)], -1)) and not (hi[~c["sk"]] >= 0).any(), loop
    for tag in ("hostile", "deleted"):
        assert out[tag + "_persist_launches"][0] >= 1 and str(out[tag + "_persist_kern"]) == "warm", out[tag + "_persist_launches"]
    assert out["hostile_sweep_best"] == out["deleted_sweep_best"]
    for lvl, (h, d) in enumerate(zip(out["hostile_sweep"], out["deleted_sweep"])):
        assert np.all(np.isfinite(h)) and h[16] == d[16], (lvl, h[16:], d[16:])
        assert synth.rel_frobenius(h[:16].reshape(4, 4), d[:16].reshape(4, 4)) < 1e-9, lvl
    bh, bd, bw = out["batch_hostile"], out["batch_deleted"], out["batch_without"]
    assert bh[0].tobytes() == bw[0].tobytes() and bh[2].tobytes() == bw[1].tobytes()
    assert np.all(np.isfinite(bh[1])) and bh[1][16] == bd[1][16] and bh[1][16] >= 0.5 * c["sk"].sum()
    assert synth.rel_frobenius(bh[1][:16].reshape(4, 4), bd[1][:16].reshape(4, 4)) < 1e-9


@pytest.mark.gpu
def test_pair_passes_over_a_hostile_search(lib, tmp_path):
    """reduce_trimmed(0.5), reduce_robust(TUKEY), reduce_gicp, reduce_information and the point-to-plane reduce over one
    search of hostile clouds, finite normals, against the same call on the deleted clouds.  (The trimmed share is
    floor(keep * ns) over EVERY source row as visma_icp_reduce_trimmed documents it: one hostile source row leaves
    floor(0.5 * 4099) = floor(0.5 * 4098) kept pairs on both sides; the target holds the 1 % scattered rows and more.)"""
    import posegraph_spec as S
    c = dict(make_case("M-tgt-mixed"))
    src = np.array(c["src"])
    _poke(src, [64], "nan1")
    c["src"], c["sk"] = src, np.isfinite(src).all(1)
    rng = np.random.default_rng(9)
    sn, tn = rng.standard_normal((len(src), 3)), rng.standard_normal((len(c["tgt"]), 3))
    sn /= np.linalg.norm(sn, axis=1, keepdims=True)
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    T0 = c["Ts"][0]
    idx, _, idx_del = reference_pass(c["src"], c["tgt"], T0, c["r"], "f64")
    assert (idx >= 0).sum() >= 0.9 * c["sk"].sum()
    s_del, t_del = deleted_clouds(c)
    out = run_probe(tmp_path, ["pairs"], {
        "r": np.array(c["r"]), "T0": T0, "hostile_src": c["src"], "hostile_tgt": c["tgt"], "hostile_sn": sn, "hostile_tn": tn,
        "deleted_src": s_del, "deleted_tgt": t_del, "deleted_sn": sn[c["sk"]], "deleted_tn": tn[c["tk"]]})
    assert np.array_equal(out["hostile_idx"], idx) and np.array_equal(out["deleted_idx"], idx_del)
    for what in ("plain", "trimmed", "robust", "gicp", "plane"):
        h, d = out["hostile_" + what], out["deleted_" + what]
        print(what, "largest relative difference %.3e" % float(np.max(np.abs(h - d) / np.maximum(np.abs(d), 1.0))))
        assert np.all(np.isfinite(h)) and stats_close(h, d), what
    assert out["hostile_plain"][0] == (idx >= 0).sum()
    paired = idx >= 0
    kept, w = out["hostile_kept"], out["hostile_weights"]
    assert np.array_equal(kept[c["sk"]], out["deleted_kept"]) and not kept[~paired].any() and kept.sum() == 4099 // 2
    assert np.array_equal(w[c["sk"]], out["deleted_weights"]) and np.all(w[~paired] == 0.0) and (w[paired] > 0).any()
    # the information sums, as tests/test_information.py compares them: against the specification, inside its bound
    M, Md = out["hostile_information"], out["deleted_information"]
    want, Sabs = S.information_terms(c["tgt"][idx[paired]].astype(np.float64))
    bound = S.information_bound(int(paired.sum()), Sabs)
    assert np.all(np.isfinite(M)) and np.all(np.abs(M - want) <= bound) and np.all(np.abs(M - Md) <= bound)


@pytest.mark.gpu
def test_a_finite_box_wider_than_fp32_can_bin_is_refused_by_the_grid_and_searched_by_brute_force(lib, oracle, tmp_path):
    """Two finite target rows at +-2e38: cell_coord's v - mn would overflow fp32.  The grid build refuses the box with
    VISMA_ICP_ERR_INVALID and says why; NN_BRUTE returns the reference's pairs (the rows' d2 overflows: never a pair)."""
    ns, nt, r, spread = SHAPES["M"]
    rng = np.random.default_rng(77)
    src, tgt = _clouds(rng, ns, nt, spread)
    tgt[3, 0], tgt[5, 0] = np.float32(2e38), np.float32(-2e38)
    T0 = synth.make_T(synth.rot_y(0.01), [0.01, -0.02, 0.005])
    idx, _, idx_del = reference_pass(src, tgt, T0, r)
    assert (idx >= 0).sum() >= 0.9 * ns
    out = run_probe(tmp_path, ["wide"], {"src": src, "tgt": tgt, "T0": T0, "r": np.array(r)})
    assert int(out["grid_error"]) == 1 and "wider than half the fp32 range" in str(out["grid_message"]), (out["grid_error"], out["grid_message"])
    assert str(out["brute_kern"]) == "brute" and np.array_equal(out["brute_idx"], idx)
    _, oidx, od2 = oracle.k_nn_pass(src, tgt, T0[:3, :].astype(np.float32), np.float32(r * r), grid=False)
    assert np.array_equal(out["brute_d2"].view(np.uint32), od2[idx >= 0].view(np.uint32))
    want = oracle.k_reduce_stats(src, tgt, idx_del, T0[:3, :])
    assert stats_close(out["brute_st"], want)
