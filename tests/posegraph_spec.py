"""A numpy specification of the multiway registration (visma_icp.h: information matrix, pose-graph optimisation), written
from Choi, Zhou, Koltun (CVPR 2015) and the description of Open3D 0.3.0's GlobalOptimization in visma_icp.h -- what
tests/test_information.py and tests/test_posegraph.py compare the library with, and what tests/golden/gen_posegraph.py
takes the margins of a run's stopping tests from.  Pinned itself to the compiled reference by tests/golden/posegraph.npz."""
import numpy as np

U = 2.0 ** -53


def information_terms(q):
    """q: K x 3 target points of the pairs -> (G^T G summed: 6 x 6, S: the sum of |term| per entry)"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    one, zero = np.ones(len(q)), np.zeros(len(q))
    rows = [np.stack([zero, z, -y, one, zero, zero], 1), np.stack([-z, zero, x, zero, one, zero], 1),
            np.stack([y, -x, zero, zero, zero, one], 1)]
    M = np.zeros((6, 6)); S = np.zeros((6, 6))
    for a in range(6):
        for b in range(6):
            t = rows[0][:, a] * rows[0][:, b] + rows[1][:, a] * rows[1][:, b] + rows[2][:, a] * rows[2][:, b]
            M[a, b] = t.sum()
            S[a, b] = np.abs(rows[0][:, a] * rows[0][:, b]).sum() + np.abs(rows[1][:, a] * rows[1][:, b]).sum() + \
                np.abs(rows[2][:, a] * rows[2][:, b]).sum()
    return M, S


def information_bound(K, S):
    """both sides sum K terms in f64 in some order: |a - b| <= 2 (K + 4) 2^-53 S per entry"""
    return 2.0 * (K + 4) * U * S


class Edge:
    def __init__(self, source, target, transformation, information, uncertain=False, confidence=1.0):
        self.source, self.target = int(source), int(target)
        self.transformation = np.array(transformation, np.float64).reshape(4, 4)
        self.information = np.array(information, np.float64).reshape(6, 6)
        self.uncertain, self.confidence = bool(uncertain), float(confidence)

    def copy(self):
        return Edge(self.source, self.target, self.transformation, self.information, self.uncertain, self.confidence)


def lin6(M):
    return np.array([(-M[1, 2] + M[2, 1]) / 2.0, (-M[2, 0] + M[0, 2]) / 2.0, (-M[0, 1] + M[1, 0]) / 2.0, M[0, 3], M[1, 3], M[2, 3]])


def _ops():
    ops = [np.zeros((4, 4)) for _ in range(6)]
    ops[0][1, 2], ops[0][2, 1] = -1, 1
    ops[1][0, 2], ops[1][2, 0] = 1, -1
    ops[2][0, 1], ops[2][1, 0] = -1, 1
    ops[3][0, 3] = ops[4][1, 3] = ops[5][2, 3] = 1
    return ops


OPS = _ops()


def zeta(poses, edges, absolute=False):
    """6 per edge: the linearised X^-1 Tt^-1 Ts; absolute: the same expression over the factors' absolute values, the
    sum of |term| a tolerance is taken relative to"""
    out = np.zeros((len(edges), 6))
    for k, e in enumerate(edges):
        Xi, Tti, Ts = np.linalg.inv(e.transformation), np.linalg.inv(poses[e.target]), poses[e.source]
        if absolute:
            M = np.abs(Xi) @ np.abs(Tti) @ np.abs(Ts)
            out[k] = [(M[1, 2] + M[2, 1]) / 2.0, (M[2, 0] + M[0, 2]) / 2.0, (M[0, 1] + M[1, 0]) / 2.0, M[0, 3], M[1, 3], M[2, 3]]
        else:
            out[k] = lin6(Xi @ Tti @ Ts)
    return out


def linear_system(poses, edges, z=None, absolute=False):
    """H (6n x 6n) and b (6n) of ComputeLinearSystem; absolute: over absolute values (the sum of |term| per entry)"""
    n = 6 * len(poses)
    H = np.zeros((n, n)); b = np.zeros(n)
    if z is None:
        z = zeta(poses, edges, absolute)
    for k, e in enumerate(edges):
        Xi, Tti, Ts = np.linalg.inv(e.transformation), np.linalg.inv(poses[e.target]), poses[e.source]
        Js = np.zeros((6, 6))
        for i in range(6):
            if absolute:
                M = np.abs(Xi) @ np.abs(Tti) @ np.abs(OPS[i]) @ np.abs(Ts)
                Js[:, i] = [(M[1, 2] + M[2, 1]) / 2.0, (M[2, 0] + M[0, 2]) / 2.0, (M[0, 1] + M[1, 0]) / 2.0, M[0, 3], M[1, 3], M[2, 3]]
            else:
                Js[:, i] = lin6(Xi @ Tti @ OPS[i] @ Ts)
        Jt = Js if absolute else -Js
        I = np.abs(e.information) if absolute else e.information
        l = e.confidence
        i0, j0 = 6 * e.source, 6 * e.target
        H[i0:i0 + 6, i0:i0 + 6] += l * Js.T @ I @ Js
        H[i0:i0 + 6, j0:j0 + 6] += l * Js.T @ I @ Jt
        H[j0:j0 + 6, i0:i0 + 6] += l * Jt.T @ I @ Js
        H[j0:j0 + 6, j0:j0 + 6] += l * Jt.T @ I @ Jt
        eI = (np.abs(z[k]) if absolute else z[k]) @ I
        if absolute:
            b[i0:i0 + 6] += l * eI @ Js; b[j0:j0 + 6] += l * eI @ Jt
        else:
            b[i0:i0 + 6] -= l * eI @ Js; b[j0:j0 + 6] -= l * eI @ Jt
    return H, b


def ldlt_solve(A, b):
    """L D L^T with diagonal pivoting as Eigen's LDLT runs it: the largest remaining diagonal entry first, no cut-off other
    than an exactly zero pivot"""
    A = np.array(A, np.float64); n = len(A)
    tr = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        tr[k] = p
        if p != k:
            A[[k, p], :k] = A[[p, k], :k]
            A[p + 1:, [k, p]] = A[p + 1:, [p, k]]
            A[k, k], A[p, p] = A[p, p], A[k, k]
            t = A[k + 1:p, k].copy(); A[k + 1:p, k] = A[p, k + 1:p]; A[p, k + 1:p] = t
        if k > 0:
            temp = np.diag(A)[:k] * A[k, :k]
            A[k, k] -= A[k, :k] @ temp
            A[k + 1:, k] -= A[k + 1:, :k] @ temp
        if k == 0 and A[0, 0] == 0.0:
            tr = np.arange(n)
            break
        if A[k, k] != 0.0:
            A[k + 1:, k] /= A[k, k]
    x = np.array(b, np.float64)
    for k in range(n):
        x[[k, tr[k]]] = x[[tr[k], k]]
    for i in range(n):
        x[i] -= A[i, :i] @ x[:i]
    d = np.diag(A)
    x = np.where(np.abs(d) > 1.0 / np.finfo(np.float64).max, x / np.where(d == 0.0, 1.0, d), 0.0)
    for i in range(n - 1, -1, -1):
        x[i] -= A[i + 1:, i] @ x[i + 1:]
    for k in range(n - 1, -1, -1):
        x[[k, tr[k]]] = x[[tr[k], k]]
    return x


def euler_zyx(v):
    ca, sa, cb, sb, cg, sg = np.cos(v[0]), np.sin(v[0]), np.cos(v[1]), np.sin(v[1]), np.cos(v[2]), np.sin(v[2])
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = v[3:]
    return T


def vec6(T):
    sy = np.sqrt(T[0, 0] * T[0, 0] + T[1, 0] * T[1, 0])
    if not sy < 1e-6:
        r = [np.arctan2(T[2, 1], T[2, 2]), np.arctan2(-T[2, 0], sy), np.arctan2(T[1, 0], T[0, 0])]
    else:
        r = [np.arctan2(-T[1, 2], T[1, 1]), np.arctan2(-T[2, 0], sy), 0.0]
    return np.array(r + [T[0, 3], T[1, 3], T[2, 3]])


class Trace:
    """every stopping test a run evaluated: (name, left side, right side, fired).  margin(): the smallest factor between
    the two sides of a test that DECIDED something -- one that fired and ended an optimisation, or the pruning of an
    uncertain edge; clearance(): the same over every test evaluated (one that did not fire must not sit within rounding
    of firing either).  Tests on integers and tests whose sides differ in sign are near nothing."""

    def __init__(self):
        self.tests = []

    def test(self, name, lhs, rhs, fired):
        self.tests.append((name, float(lhs), float(rhs), bool(fired)))
        return fired

    def _factor(self, tests):
        m = np.inf
        for name, lhs, rhs, _ in tests:
            if lhs <= 0.0 or rhs <= 0.0 or name.startswith("max iteration"):
                continue
            m = min(m, max(lhs / rhs, rhs / lhs))
        return m

    def margin(self):
        return self._factor([t for t in self.tests if t[3] or t[0] == "prune"])

    def clearance(self):
        return self._factor(self.tests)

    def deciding(self):
        fired = [t for t in self.tests if t[3]]
        return fired[-1] if fired else None


DEFAULT_CRITERIA = dict(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6, min_right_term=1e-6,
                        min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2. / 3., lower_scale_factor=1. / 3.)
DEFAULT_OPTION = dict(max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1)


def clamp_option(o):
    o = dict(DEFAULT_OPTION, **(o or {}))
    if o["max_correspondence_distance"] < 0.0:
        o["max_correspondence_distance"] = 0.075
    if o["edge_prune_threshold"] < 0.0 or o["edge_prune_threshold"] > 1.0:
        o["edge_prune_threshold"] = 0.25
    if o["preference_loop_closure"] < 0.0:
        o["preference_loop_closure"] = 1.0
    return o


def clamp_criteria(c):
    c = dict(DEFAULT_CRITERIA, **(c or {}))
    if c["upper_scale_factor"] < 0.0 or c["upper_scale_factor"] > 1.0:
        c["upper_scale_factor"] = 2. / 3.
    if c["lower_scale_factor"] < 0.0 or c["lower_scale_factor"] > 1.0:
        c["lower_scale_factor"] = 1. / 3.
    return c


def validate(n_nodes, edges):
    for i in range(n_nodes - 1):
        if not any(e.source == i and e.target - e.source == 1 for e in edges):
            return False
    return all(0 <= e.source < n_nodes and 0 <= e.target < n_nodes for e in edges)


def _optimize(poses, edges, method, c, o, tr):
    n = 6 * len(poses)
    if n == 0:
        return poses, edges
    w = o["preference_loop_closure"] * o["max_correspondence_distance"] ** 2 * (np.mean([e.information[5, 5] for e in edges]) if edges else 0.0)

    def residual(z):
        return sum(e.confidence * (z[k] @ e.information @ z[k]) + w * (np.sqrt(e.confidence) - 1) ** 2 for k, e in enumerate(edges))

    def update_confidence(z):
        for k, e in enumerate(edges):
            t = w / (w + z[k] @ e.information @ z[k])
            e.confidence = t * t

    z = zeta(poses, edges)
    cur = residual(z)
    update_confidence(z)
    x = np.concatenate([vec6(T) for T in poses])
    H, b = linear_system(poses, edges, z)
    right = lambda: tr.test("right term", b.max(), c["min_right_term"], b.max() < c["min_right_term"])
    incr = lambda d: tr.test("relative increment", np.linalg.norm(d), c["min_relative_increment"] * (np.linalg.norm(x) + c["min_relative_increment"]),
                             np.linalg.norm(d) < c["min_relative_increment"] * (np.linalg.norm(x) + c["min_relative_increment"]))
    resincr = lambda new: tr.test("relative residual increment", cur - new, c["min_relative_residual_increment"] * cur,
                                  cur - new < c["min_relative_residual_increment"] * cur)
    if right():
        return poses, edges
    stop = False
    it = 0
    lam = 1e-5 * np.diag(H).max(); ni = 2.0; rho = 0.0
    while not stop:
        if method == 0:
            d = ldlt_solve(H, b)
            if incr(d):
                break
            new_poses = [euler_zyx(d[6 * i:6 * i + 6]) @ T for i, T in enumerate(poses)]
            zn = zeta(new_poses, edges)
            new = residual(zn)
            if resincr(new):
                break
            cur, z, poses = new, zn, new_poses
            x = np.concatenate([vec6(T) for T in poses])
            update_confidence(z)
            H, b = linear_system(poses, edges, z)
            if right():
                break
        else:
            lm = 0
            while True:
                d = ldlt_solve(H + lam * np.eye(n), b)
                stop = stop or incr(d)
                if not stop:
                    new_poses = [euler_zyx(d[6 * i:6 * i + 6]) @ T for i, T in enumerate(poses)]
                    zn = zeta(new_poses, edges)
                    new = residual(zn)
                    rho = (cur - new) / (d @ (lam * d + b) + 1e-3)
                    if rho > 0:
                        stop = stop or resincr(new)
                        if stop:
                            break
                        alpha = min(1. - (2 * rho - 1) ** 3, c["upper_scale_factor"])
                        lam *= max(c["lower_scale_factor"], alpha)
                        ni = 2.0
                        cur, z, poses = new, zn, new_poses
                        x = np.concatenate([vec6(T) for T in poses])
                        update_confidence(z)
                        H, b = linear_system(poses, edges, z)
                        stop = stop or right()
                        if stop:
                            break
                    else:
                        lam *= ni; ni *= 2
                lm += 1
                stop = stop or tr.test("max iteration (LM)", lm, c["max_iteration_lm"], lm >= c["max_iteration_lm"])
                if rho > 0 or stop:
                    break
        stop = stop or tr.test("residual", cur, c["min_residual"], cur < c["min_residual"])
        stop = stop or tr.test("max iteration", it, c["max_iteration"], it >= c["max_iteration"])
        it += 1
    return poses, edges


def global_optimization(poses, edges, method="lm", criteria=None, option=None):
    """-> (poses, surviving edges, Trace).  An invalid graph comes back as given."""
    m = {"gn": 0, "lm": 1}[method] if isinstance(method, str) else int(method)
    c, o = clamp_criteria(criteria), clamp_option(option)
    tr = Trace()
    orig = [np.array(T, np.float64).reshape(4, 4) for T in poses]
    edges = [e.copy() for e in edges]
    if not validate(len(orig), edges):
        return orig, edges, tr
    p1, e1 = _optimize(list(orig), edges, m, c, o, tr)
    for e in e1:                                           # (a confidence lies in [0, 1]: a kept edge's distance is taken from 1)
        if e.uncertain and e.confidence > o["edge_prune_threshold"]:
            tr.test("prune", 1.0 - o["edge_prune_threshold"], 1.0 - e.confidence, False)
        elif e.uncertain:
            tr.test("prune", e.confidence, o["edge_prune_threshold"], False)
    kept = [e for e in e1 if (not e.uncertain) or e.confidence > o["edge_prune_threshold"]]
    p2, e2 = _optimize(p1, kept, m, c, o, tr)
    r = o["reference_node"]
    if 0 <= r < len(p2):
        comp = orig[r] @ np.linalg.inv(p2[r])
        p2 = [comp @ T for T in p2]
    return p2, e2, tr
