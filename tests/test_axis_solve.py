"""The updates constrained to a rotation about one axis plus a translation (visma_icp_solve_from_stats_axis,
host_math.hpp: kabsch_axis_from_stats / gn_axis_from_stats) against an independent restatement in numpy from the raw
pairs -- not from the 38 statistics: the centred pairs projected onto the plane normal to the axis give the angle by
atan2.  CPU only: the solves are host code (the device runs the same functions)."""
import numpy as np
import pytest

AXES = [np.array(v, float) for v in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])]


def hat(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def rot(a, th):
    a = a / np.linalg.norm(a)
    return np.cos(th) * np.eye(3) + np.sin(th) * hat(a) + (1 - np.cos(th)) * np.outer(a, a)


def pp_stats(p, q):
    """the 38 point-to-point statistics of the pairs (layout of device_common.h: expand_moments), in f64"""
    K = len(p)
    P, Q = p.sum(0), q.sum(0)
    S = p.T @ p
    M = q.T @ p                                    # sum q p^T
    J = np.zeros((6, 6))
    J[:3, :3] = np.trace(S) * np.eye(3) - S
    J[:3, 3:] = hat(P)
    J[3:, :3] = hat(P).T
    J[3:, 3:] = K * np.eye(3)
    st = np.zeros(38)
    st[0] = K
    st[1] = float(((p - q) ** 2).sum())
    st[2:23] = J[np.triu_indices(6)]
    st[23:26] = -np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2.0
    st[26:29] = P - Q
    st[29:38] = M.reshape(9)
    return st


def pl_stats(p, q, n):
    """the point-to-plane statistics: J rows [p x n, n], r = (p - q) . n"""
    J = np.c_[np.cross(p, n), n]
    r = ((p - q) * n).sum(1)
    st = np.zeros(38)
    st[0] = len(p)
    st[1] = float(((p - q) ** 2).sum())
    st[2:23] = (J.T @ J)[np.triu_indices(6)]
    st[23:29] = J.T @ r
    return st


def basis(a):
    """u, v with u x v = a (a unit)"""
    e = np.eye(3)[int(np.argmin(np.abs(a)))]
    u = np.cross(a, e)
    u /= np.linalg.norm(u)
    return u, np.cross(a, u)


def restated(p, q, a):
    """the 4-DoF least-squares answer from the raw pairs: angle in the plane normal to a, t = qm - R pm"""
    a = a / np.linalg.norm(a)
    pm, qm = p.mean(0), q.mean(0)
    pc, qc = p - pm, q - qm
    u, v = basis(a)
    pu, pv, qu, qv = pc @ u, pc @ v, qc @ u, qc @ v
    th = np.arctan2((pu * qv - pv * qu).sum(), (pu * qu + pv * qv).sum())
    R = rot(a, th)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = qm - R @ pm
    return T, th


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def angle_of(R, a):
    """the angle of a rotation about the unit axis a"""
    return np.arctan2(0.5 * np.dot(a, [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]), 0.5 * (np.trace(R) - 1.0))


def cases(rng, n_cases=200):
    out = []
    for k in range(n_cases):
        n = int(rng.integers(3, 5001))
        if k < 2 * len(AXES):
            a = AXES[k % len(AXES)]
        else:
            a = rng.standard_normal(3)
            a /= np.linalg.norm(a)
        th = rng.uniform(-np.pi, np.pi)
        if k == 0:
            th = np.pi
        t = rng.standard_normal(3) * 0.5
        p = rng.standard_normal((n, 3)) * rng.uniform(0.2, 2.0, 3) + rng.standard_normal(3) * 0.3
        noise = 0.0 if k % 5 == 0 else 10.0 ** rng.uniform(-6, -2)
        q = p @ rot(a, th).T + t + rng.standard_normal((n, 3)) * noise
        out.append((k, a, th, t, noise, p, q))
    return out


def test_closed_form_matches_restatement(lib):
    rng = np.random.default_rng(11)
    worst = 0.0
    for k, a, th, t, noise, p, q in cases(rng):
        T = lib.solve_from_stats_axis(pp_stats(p, q), a)
        Tref, _ = restated(p, q, a)
        e = rel(T, Tref)
        worst = max(worst, e)
        assert e < 1e-12, (k, len(p), e)
    print("worst relative difference: %.2e" % worst)


def test_exact_yaw_data_gives_back_its_motion(lib):
    rng = np.random.default_rng(12)
    for k, a, th, t, noise, p, q in cases(rng, 60):
        if noise != 0.0:
            continue
        T = lib.solve_from_stats_axis(pp_stats(p, q), a)
        dth = np.angle(np.exp(1j * (angle_of(T[:3, :3], a) - th)))
        assert abs(dth) < 1e-12, (k, dth)
        assert np.max(np.abs(T[:3, 3] - t)) < 1e-12, (k, T[:3, 3] - t)


def test_closed_form_is_optimal_over_a_grid(lib):
    rng = np.random.default_rng(13)
    grid = np.linspace(-np.pi, np.pi, 7201)[1:]                    # 7,200 angles over (-pi, pi]
    for k, a, th, t, noise, p, q in cases(rng, 24):
        T = lib.solve_from_stats_axis(pp_stats(p, q), a)
        pc, qc = p - p.mean(0), q - q.mean(0)
        Cm = qc.T @ pc                                             # sum qc pc^T
        base = float((pc ** 2).sum() + (qc ** 2).sum())
        # objective with the best t at each angle: base - 2 tr(R^T C), R = c I + s [a]x + (1 - c) a a^T
        c, s = np.cos(grid), np.sin(grid)
        f_grid = base - 2.0 * (c * np.trace(Cm) + s * (hat(a) * Cm).sum() + (1 - c) * (a @ Cm @ a))
        f_lib = float(((p @ T[:3, :3].T + T[:3, 3] - q) ** 2).sum())
        assert f_lib <= f_grid.min() + 1e-9 * max(base, 1.0), (k, f_lib, f_grid.min())


def test_result_is_a_rotation_about_the_axis(lib):
    rng = np.random.default_rng(14)
    for k, a, th, t, noise, p, q in cases(rng, 100):
        R = lib.solve_from_stats_axis(pp_stats(p, q), a)[:3, :3]
        assert np.max(np.abs(R @ a - a)) <= 1e-15, k
        assert np.max(np.abs(R.T @ R - np.eye(3))) <= 1e-15, k
        assert abs(np.linalg.det(R) - 1.0) <= 1e-15, k


def test_degenerate_inputs(lib):
    # no correspondences
    assert np.array_equal(lib.solve_from_stats_axis(np.zeros(38), [0, 1, 0]), np.eye(4))
    assert np.array_equal(lib.solve_from_stats_axis(np.zeros(38), [0, 1, 0], plane=True), np.eye(4))
    rng = np.random.default_rng(15)
    # every point on a line parallel to the axis: the angle is undetermined -> no rotation, t = qm - pm
    for a in AXES[:3] + [np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])]:
        s = rng.standard_normal((300, 1))
        p = np.array([0.4, -0.7, 1.1]) + s * a
        q = p @ rot(a, 0.8).T + np.array([0.1, 0.2, -0.3])
        T = lib.solve_from_stats_axis(pp_stats(p, q), a)
        assert np.allclose(T[:3, :3], np.eye(3), atol=0, rtol=0), a
        assert np.max(np.abs(T[:3, 3] - (q.mean(0) - p.mean(0)))) < 1e-12
    # a non-unit axis is normalised
    p = rng.standard_normal((500, 3))
    a = np.array([0.3, 1.0, -0.2])
    q = p @ rot(a, 0.4).T + 0.05
    st = pp_stats(p, q)
    T1 = lib.solve_from_stats_axis(st, a * 7.5)
    T2 = lib.solve_from_stats_axis(st, a / np.linalg.norm(a))
    assert np.max(np.abs(T1 - T2)) < 1e-15
    for plane in (False, True):
        for bad in ([0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1e-14, 0, 0]):
            with pytest.raises(lib.IcpError):
                lib.solve_from_stats_axis(st, bad, plane=plane)


def test_point_to_plane_step_matches_numpy(lib):
    rng = np.random.default_rng(16)
    worst = 0.0
    for k in range(60):
        n = int(rng.integers(10, 3000))
        a = AXES[k % len(AXES)] if k < 12 else rng.standard_normal(3)
        a = a / np.linalg.norm(a)
        p = rng.standard_normal((n, 3)) + rng.standard_normal(3) * 0.3
        nr = rng.standard_normal((n, 3))
        nr /= np.linalg.norm(nr, axis=1, keepdims=True)
        q = p @ rot(a, rng.uniform(-0.3, 0.3)).T + rng.standard_normal(3) * 0.05 + rng.standard_normal((n, 3)) * 1e-3
        T = lib.solve_from_stats_axis(pl_stats(p, q, nr), a, plane=True)
        # numpy: the 4-column Jacobian ((p x n) . a, n)
        J4 = np.c_[np.cross(p, nr) @ a, nr]
        r = ((p - q) * nr).sum(1)
        y = np.linalg.solve(J4.T @ J4, -(J4.T @ r))
        Tref = np.eye(4)
        Tref[:3, :3] = rot(a, y[0])
        Tref[:3, 3] = y[1:]
        e = rel(T, Tref)
        worst = max(worst, e)
        assert e < 1e-12, (k, e)
        assert np.max(np.abs(T[:3, :3] @ a - a)) < 1e-15
    print("worst relative difference: %.2e" % worst)


def test_point_to_plane_floor_only_is_rejected_by_the_guard(lib):
    # every normal equals the axis: the angle has no leverage (column 0 of J is 0) -> det H = 0 -> identity
    rng = np.random.default_rng(17)
    for a in AXES[2:4] + [np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])]:
        p = rng.standard_normal((400, 3))
        nr = np.tile(a, (400, 1))
        q = p + 0.01
        T = lib.solve_from_stats_axis(pl_stats(p, q, nr), a, plane=True)
        assert np.array_equal(T, np.eye(4)), a
