"""One object through a history of calls against fresh objects (the pattern of tests/test_buffer_reuse.py, for every object
that lives across calls; tests/test_history.py).

The rule: a call's result depends on the object's logical state (the cloud, the voxels, the mesh, the images and poses) and
on the call's arguments -- never on what the object computed before.  replay() runs the calls of a history in order on ONE
object and, for every call, on an object made fresh and brought to the same logical state by the shortest route; the two
results must be the same bytes.  GPU against GPU on one machine: raw bytes, no NaN canonicalisation, no tolerance."""
import numpy as np


def flatten(result):
    """a call's result (arrays, ints, error codes, None, nested tuples / lists / dicts of them) -> a flat list of (path, item)"""
    out = []

    def walk(path, r):
        if isinstance(r, dict):
            for k in sorted(r):
                walk("%s[%r]" % (path, k), r[k])
        elif isinstance(r, (tuple, list)):
            for i, x in enumerate(r):
                walk("%s[%d]" % (path, i), x)
        else:
            out.append((path, r))
    walk("", result)
    return out


def _rows(a):
    a = np.ascontiguousarray(a)
    return a.reshape(len(a), -1) if a.ndim else a.reshape(1, 1)


def difference(got, want):
    """None if two results are the same -- dtype, shape and bytes of every array, value of everything else --, else a line
    that names the first item that differs and its first differing rows"""
    g, w = flatten(got), flatten(want)
    if [p for p, _ in g] != [p for p, _ in w]:
        return "the results have another structure: %s against %s" % ([p for p, _ in g], [p for p, _ in w])
    for (path, a), (_, b) in zip(g, w):
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)):
                return "item %s: %s against %s" % (path, type(a).__name__, type(b).__name__)
            if a.dtype != b.dtype or a.shape != b.shape:
                return "item %s: %s %s against %s %s" % (path, a.dtype, a.shape, b.dtype, b.shape)
            if a.tobytes() == b.tobytes():
                continue
            ra, rb = _rows(a), _rows(b)
            bad = np.nonzero((ra.view(np.uint8).reshape(len(ra), -1) != rb.view(np.uint8).reshape(len(rb), -1)).any(axis=1))[0]
            cols = np.nonzero((ra[bad[:3]] != rb[bad[:3]]).any(axis=0) | (ra[bad[:3]] != ra[bad[:3]]).any(axis=0))[0][:6]
            return "item %s: %d of %d rows differ, first rows %s, columns %s: with a history %s, fresh %s" % (
                path, len(bad), len(ra), bad[:5].tolist(), cols.tolist(), ra[bad[:3]][:, cols].tolist(), rb[bad[:3]][:, cols].tolist())
        if a is None or b is None:
            if a is not b:
                return "item %s: %r against %r" % (path, a, b)
        elif type(a) is not type(b) or a != b:
            return "item %s: %r against %r" % (path, a, b)
    return None


def replay(make, steps, close=None):
    """make() -> a new object; steps: a list of (name, to_state, call).  to_state(obj) brings a FRESH object to the logical
    state the step expects (None: the call is stateless); call(obj) -> a tuple of numpy arrays, ints and error codes.

    Every call runs in order on one object.  For each step a fresh object is also made, brought to the state, given the call
    and closed, and the two results are compared: dtype, shape and bytes.  The first step that differs fails by name with its
    first differing rows.  -> the fresh results, in the steps' order.  close(obj) defaults to obj.close()."""
    close = close or (lambda obj: obj.close())
    fresh_results = []
    reused = make()
    try:
        for k, (name, to_state, call) in enumerate(steps):
            got = call(reused)
            fresh = make()
            try:
                if to_state is not None:
                    to_state(fresh)
                want = call(fresh)
            finally:
                close(fresh)
            diff = difference(got, want)
            assert diff is None, "step %d (%s) differs from a fresh object: %s" % (k, name, diff)
            fresh_results.append(want)
    finally:
        close(reused)
    return fresh_results
