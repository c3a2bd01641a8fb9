"""The GPU body of tests/test_core_hostile.py: runs the registration core on the clouds it is handed and writes down what
came back.  It judges nothing -- the reference, the remapping and every assertion live in the test, which starts one
child per search policy (the policies are partly chosen by environment variables read when a context is created).

usage: core_hostile_probe.py search KERNEL UPLOAD in.npz out.npz      five passes per case, twice (determinism)
       core_hostile_probe.py loops  in.npz out.npz                    run / iterate / device loop / persistent loop / yaw sweep / batch
       core_hostile_probe.py pairs  in.npz out.npz                    the pair passes over one search
       core_hostile_probe.py wide   in.npz out.npz                    a finite box wider than fp32 can bin: grid error, brute force
KERNEL: brute | serial | auto | warm | ring | exact      UPLOAD: f32 | device | f64
in.npz: names, and per case i: {i}_src, {i}_tgt (fp32, n x 3), {i}_Ts (passes x 4 x 4), {i}_r (+ what a mode adds)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from visma_amd import _lib  # noqa: E402

PERSIST_TIMEOUT_MS = 200.0       # finite: a launch whose loop did not end comes back as an error, not as a hang


def make_ctx(kernel):
    for k in ("VISMA_ICP_COOP", "VISMA_ICP_GRID_LANES"):
        os.environ.pop(k, None)
    if kernel == "serial":                                   # the lane-serial kernel, one query per lane, every pass
        os.environ["VISMA_ICP_COOP"] = "0"
        os.environ["VISMA_ICP_GRID_LANES"] = "801"
    c = _lib.Context(0)
    prec, mode, ring = {"brute": ("f32", _lib.NN_BRUTE, 0), "serial": ("f32", _lib.NN_GRID, 0),
                        "auto": ("f32", _lib.NN_AUTO, 0), "warm": ("exact", _lib.NN_GRID, 0),
                        "ring": ("exact", _lib.NN_GRID, 1), "exact": ("exact", _lib.NN_AUTO, -1)}[kernel]
    c.set_search_precision(prec)
    c.set_nn_mode(mode)
    c.set_ring_search(ring)
    if kernel == "warm":
        c.set_persistent(False)
    return c


_alive = []
_torch = None                # decided before the first context exists: torch must initialise its runtime first, if at all
_hip = None


def device_setup():
    """Device memory the library did not allocate: a torch tensor where torch sees the GPU in this process, else a
    plain hipMalloc through the HIP runtime (said in the output: `device_via`)."""
    global _torch, _hip
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1).cuda()
            torch.cuda.synchronize()
            _torch = torch
            return "torch"
    except Exception:
        pass
    import ctypes
    _hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")              # (the runtime the library itself is linked against)
    _hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return "hipMalloc"


def device_copy(xyzw):
    if _torch is not None:
        t = _torch.from_numpy(xyzw).cuda()
        _torch.cuda.synchronize()
        _alive.append(t)
        return t.data_ptr()
    import ctypes
    p = ctypes.c_void_p()
    assert _hip.hipMalloc(ctypes.byref(p), xyzw.nbytes) == 0
    assert _hip.hipMemcpy(p, xyzw.ctypes.data_as(ctypes.c_void_p), xyzw.nbytes, 1) == 0      # hipMemcpyHostToDevice
    _alive.append(p)                                         # (a few MB, left to the end of this process)
    return p.value


def upload(c, src, tgt, how):
    if how == "f32":
        c.set_target(tgt)
        c.set_source(src)
    elif how == "f64":
        c.set_clouds_f64(src.astype(np.float64), tgt.astype(np.float64))
    elif how == "device":
        del _alive[:]
        for a, put in ((tgt, c.set_target_device), (src, c.set_source_device)):
            xyzw = np.zeros((max(len(a), 1), 4), np.float32)
            xyzw[:len(a), :3] = a
            put(device_copy(xyzw), len(a))                   # (the context makes its own copy inside the call)
    else:
        raise ValueError(how)


def one_pass(c, T, r):
    c.nn_pass(T, r)
    st = c.reduce()
    si, ti, d2 = c.get_correspondences()
    idx = np.full(c.ns, -1, np.int32)
    idx[si] = ti
    return idx, d2, st


def search(kernel, how, cin, out):
    if how == "device":
        out["device_via"] = np.array(device_setup())
    c = make_ctx(kernel)
    for i, _name in enumerate(cin["names"]):
        src, tgt, Ts, r = cin["%d_src" % i], cin["%d_tgt" % i], cin["%d_Ts" % i], float(cin["%d_r" % i])
        for rep in (0, 1):
            upload(c, src, tgt, how)
            for p, T in enumerate(Ts):
                idx, d2, st = one_pass(c, T, r)
                key = "%d_%d_%d_" % (i, p, rep)
                out[key + "idx"], out[key + "d2"], out[key + "st"] = idx, d2, st
                out[key + "kern"] = np.array(c.search_kernel_used())
    c.close()


def result_row(r):
    return np.concatenate([np.asarray(r.transformation_, np.float64).ravel(),
                           [r.num_correspondences, r.fitness_, r.inlier_rmse_, r.iterations]])


def loops(cin, out):
    r, T0, iters = float(cin["r"]), cin["T0"], 10
    for tag in ("hostile", "deleted"):
        src, tgt = cin[tag + "_src"], cin[tag + "_tgt"]
        c = _lib.Context(0)
        c.set_nn_mode(_lib.NN_GRID)
        c.set_ring_search(0)
        upload(c, src, tgt, "f32")
        # the host loop, one launch per pass
        c.set_device_loop(False)
        c.set_persistent(False)
        out[tag + "_run"] = result_row(c.run(T0, r, iters, 0.0, 0.0))
        out[tag + "_run_idx"] = c.correspondence_index()
        c.forget_winners()
        T, last = c.iterate(T0, r, iters)
        out[tag + "_iterate"] = np.concatenate([T.ravel(), [last.num_correspondences, last.fitness_, last.inlier_rmse_, iters]])
        # the same loop inside the persistent launch
        c.set_persistent(True, PERSIST_TIMEOUT_MS)
        c.forget_winners()
        before = c.persistent_info()["launches"]
        out[tag + "_persist"] = result_row(c.run(T0, r, iters, 0.0, 0.0))
        out[tag + "_persist_idx"] = c.correspondence_index()
        info = c.persistent_info()
        out[tag + "_persist_launches"] = np.array([info["launches"] - before, info["aborts"]], np.float64)
        out[tag + "_persist_kern"] = np.array(c.search_kernel_used())
        # the loop on the device
        c.set_persistent(False)
        c.set_device_loop(True)
        c.forget_winners()
        out[tag + "_device"] = result_row(c.run(T0, r, iters, 0.0, 0.0))
        out[tag + "_device_idx"] = c.correspondence_index()
        c.set_device_loop(None)
        # four yaw starts advanced together (the wave kernel)
        _best, bl, per = c.run_yaw_sweep(4, r, iters, 0.0, 0.0)
        out[tag + "_sweep"] = np.stack([result_row(x) for x in per])
        out[tag + "_sweep_best"] = np.array(bl)
        c.close()
    # three problems in one batch, the middle one with a hostile source; the same with its rows deleted; and without it
    c = _lib.Context(0)
    A = (cin["bA_src"].astype(np.float64), cin["bA_tgt"].astype(np.float64), T0, r)
    B = (cin["hostile_src"].astype(np.float64), cin["bB_tgt"].astype(np.float64), T0, r)
    Bd = (cin["deleted_src"].astype(np.float64), cin["bB_tgt"].astype(np.float64), T0, r)
    Cc = (cin["bC_src"].astype(np.float64), cin["bC_tgt"].astype(np.float64), T0, r)
    for tag, probs in (("batch_hostile", [A, B, Cc]), ("batch_deleted", [A, Bd, Cc]), ("batch_without", [A, Cc])):
        out[tag] = np.stack([result_row(x) for x in c.run_batch(probs, max_iter=iters, rel_fitness=0.0, rel_rmse=0.0)])
    c.close()


def pairs(cin, out):
    r, T0 = float(cin["r"]), cin["T0"]
    for tag in ("hostile", "deleted"):
        src, tgt = cin[tag + "_src"], cin[tag + "_tgt"]
        c = _lib.Context(0)
        c.set_nn_mode(_lib.NN_GRID)
        upload(c, src, tgt, "f32")
        c.set_target_normals_f64(cin[tag + "_tn"])
        c.set_source_normals_f64(cin[tag + "_sn"])
        c.nn_pass(T0, r)
        out[tag + "_plain"] = c.reduce()
        out[tag + "_idx"] = c.correspondence_index()
        st, info = c.reduce_trimmed(0.5)
        out[tag + "_trimmed"], out[tag + "_kept"] = st, c.kept_mask()
        st, info = c.reduce_robust("tukey")
        out[tag + "_robust"], out[tag + "_weights"] = st, c.pair_weights()
        st, info = c.reduce_gicp()
        out[tag + "_gicp"] = st
        out[tag + "_information"] = c.reduce_information()
        st, info = c.reduce_robust("l2", plane=True)         # (w = 1: the point-to-plane statistics)
        out[tag + "_plane"] = st
        out[tag + "_kern"] = np.array(c.search_kernel_used())
        c.close()


def wide(cin, out):
    """a box of finite coordinates too wide for fp32 binning: what the grid search says, what brute force finds"""
    src, tgt, T, r = cin["src"], cin["tgt"], cin["T0"], float(cin["r"])
    c = make_ctx("serial")
    upload(c, src, tgt, "f32")
    try:
        c.nn_pass(T, r)
        out["grid_error"], out["grid_message"] = np.array(0), np.array("")
    except _lib.IcpError as e:
        out["grid_error"], out["grid_message"] = np.array(e.code), np.array(str(e))
    c.close()
    c = make_ctx("brute")
    upload(c, src, tgt, "f32")
    out["brute_idx"], out["brute_d2"], out["brute_st"] = one_pass(c, T, r)
    out["brute_kern"] = np.array(c.search_kernel_used())
    c.close()


def main():
    mode = sys.argv[1]
    out = {}
    if mode == "search":
        kernel, how, fin, fout = sys.argv[2:6]
        search(kernel, how, np.load(fin), out)
    else:
        fin, fout = sys.argv[2:4]
        {"loops": loops, "pairs": pairs, "wide": wide}[mode](np.load(fin), out)
    np.savez(fout, **out)
    print("core_hostile_probe %s: %d arrays" % (" ".join(sys.argv[1:-2]), len(out)))


if __name__ == "__main__":
    main()
