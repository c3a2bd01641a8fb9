"""A fixture of many small arrays as a few large ones.  An .npz entry costs a few hundred bytes whatever it holds, and a
fixture of a thousand digests, counts and 6 x 6 matrices is mostly that.  save() lays all arrays of one dtype end to end
(data_<dtype>) and keeps their names, dtypes, shapes and offsets beside them; load() gives the dict of arrays back."""
import numpy as np


def save(path, arrays):
    names = sorted(arrays)
    by_type, rows = {}, []
    for name in names:
        a = np.asarray(arrays[name])                                  # (ascontiguousarray would make a scalar a vector)
        assert a.ndim <= 4 and a.dtype.kind in "fiub", (name, a.dtype, a.shape)
        t = a.dtype.str.lstrip("<|=")
        flat = by_type.setdefault(t, [])
        rows.append((t, a.ndim, a.shape + (0,) * (4 - a.ndim), sum(len(f) for f in flat)))
        flat.append(a.ravel())
    out = {"data_" + t: np.concatenate(parts) for t, parts in by_type.items()}
    out["names"] = np.array(names)
    out["dtypes"] = np.array([r[0] for r in rows])
    out["shapes"] = np.array([(r[1],) + r[2] + (r[3],) for r in rows], np.int64)       # ndim, four extents, offset
    np.savez_compressed(path, **out)


def load(path):
    z = np.load(path)
    data = {k[5:]: z[k] for k in z.files if k.startswith("data_")}
    out = {}
    for name, t, row in zip(z["names"].tolist(), z["dtypes"].tolist(), z["shapes"].tolist()):
        shape = tuple(row[1:1 + row[0]])
        n = int(np.prod(shape, dtype=np.int64))
        out[name] = data[t][row[5]:row[5] + n].reshape(shape).copy()
    return out
