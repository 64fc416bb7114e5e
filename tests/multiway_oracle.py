"""numpy restatement of gcl_amd/lib/multiway.py (DESIGN.md "Multiway registration"): open3d's
get_information_matrix_from_point_clouds and global_optimization with GlobalOptimizationLevenbergMarquardt, from its
published source.  numpy only.

``information(source, target, T, distance)`` -> (info [6, 6], A [6, 6], n_corr, radius margin): the correspondences are the
brute-force rule of tests/icp_oracle.py; every element is assembled from the ten sums n, sum q, sum q q^T of the TARGET points,
as the kernel does; A is the same assembly over the absolute values of the terms.  ``information_direct`` is sum G^T G.

``global_optimization(graph, ..., dtype)`` runs the optimiser in ``dtype`` (float64 or longdouble; the L D L^T is written as
loops so that it does) and returns a dict: ``poses`` [n, 4, 4], ``confidence`` [m], ``kept`` [m], ``solves`` (pass 1, pass 2),
``residual``, ``status`` and ``margins``: the smallest relative margin |a - b| / max(|a|, |b|) of every comparison of a kind.
A graph is a dict ``nodes`` [n, 4, 4], ``edges`` [(s, t)], ``T`` [m, 4, 4], ``info`` [m, 6, 6], ``uncertain`` [m].
"""
import numpy as np

import icp_oracle

DEFAULT_CRITERIA = dict(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                        min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0,
                        lower_scale_factor=1.0 / 3.0)


# ---- information matrix -----------------------------------------------------------------------------------------------
def _assemble(n, s, S):
    """The 6 x 6 from n, s = sum q [3], S = sum q q^T [3, 3] (rotation part first)."""
    x, y, z = s
    I = np.zeros((6, 6))
    I[0, 0], I[1, 1], I[2, 2] = S[2, 2] + S[1, 1], S[2, 2] + S[0, 0], S[1, 1] + S[0, 0]
    I[0, 1] = I[1, 0] = -S[0, 1]
    I[0, 2] = I[2, 0] = -S[0, 2]
    I[1, 2] = I[2, 1] = -S[1, 2]
    I[0, 4] = I[4, 0] = -z
    I[0, 5] = I[5, 0] = y
    I[1, 3] = I[3, 1] = z
    I[1, 5] = I[5, 1] = -x
    I[2, 3] = I[3, 2] = -y
    I[2, 4] = I[4, 2] = x
    I[3, 3] = I[4, 4] = I[5, 5] = n
    return I


def correspondences(source, target, T, distance):
    x = np.asarray(source, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    q = np.asarray(target, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64)
    # p = T x in the kernel's order: ((m0 x0 + m1 x1) + m2 x2) + m3
    p = ((T[:3, 0] * x[:, 0:1] + T[:3, 1] * x[:, 1:2]) + T[:3, 2] * x[:, 2:3]) + T[:3, 3]
    corr, _, _, rad = icp_oracle.nearest(p, q, float(distance) ** 2)
    return corr, q, rad


def information(source, target, T, distance):
    corr, q, rad = correspondences(source, target, T, distance)
    qq = q[corr[corr >= 0]]
    n = len(qq)
    s = qq.sum(axis=0) if n else np.zeros(3)
    S = (qq[:, :, None] * qq[:, None, :]).sum(axis=0) if n else np.zeros((3, 3))
    a = np.abs(qq)
    sa = a.sum(axis=0) if n else np.zeros(3)
    Sa = (a[:, :, None] * a[:, None, :]).sum(axis=0) if n else np.zeros((3, 3))
    return _assemble(float(n), s, S), np.abs(_assemble(float(n), sa, Sa)), n, rad


def information_direct(source, target, T, distance):
    corr, q, _ = correspondences(source, target, T, distance)
    I = np.zeros((6, 6))
    for x, y, z in q[corr[corr >= 0]]:
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]], dtype=np.float64)
        I += G.T @ G
    return I


# ---- pose graph ----------------------------------------------------------------------------------------------------------
def rigid_inv(T):
    out = np.zeros((4, 4), dtype=T.dtype)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    out[3, 3] = 1
    return out


def lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]],
                    dtype=M.dtype)


def vec2mat(v):
    sa, ca, sb, cb, sc, cc = np.sin(v[0]), np.cos(v[0]), np.sin(v[1]), np.cos(v[1]), np.sin(v[2]), np.cos(v[2])
    M = np.zeros((4, 4), dtype=v.dtype)
    M[0, :3] = [cb * cc, sa * sb * cc - ca * sc, ca * sb * cc + sa * sc]
    M[1, :3] = [cb * sc, sa * sb * sc + ca * cc, ca * sb * sc - sa * cc]
    M[2, :3] = [-sb, sa * cb, ca * cb]
    M[:3, 3] = v[3:]
    M[3, 3] = 1
    return M


def _generators(dt):
    G = np.zeros((6, 4, 4), dtype=dt)
    for i in range(3):
        a, c = (i + 1) % 3, (i + 2) % 3
        G[i, a, c], G[i, c, a] = -1, 1
        G[3 + i, i, 3] = 1
    return G


def ldlt_solve(A, b):
    """(H + lambda I) delta = b by L D L^T without pivoting, right-looking, in A's dtype; None at a pivot <= 0."""
    n = len(b)
    L = A.copy()
    for j in range(n):
        d = L[j, j]
        if not (d > 0 and np.isfinite(d)):
            return None
        col = L[j + 1:, j].copy()
        L[j + 1:, j] = col / d
        for i in range(j + 1, n):
            L[i, j + 1:i + 1] -= L[i, j] * col[:i - j]
    y = b.copy()
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    x = y / np.diag(L)
    for j in range(n - 1, 0, -1):
        x[:j] -= L[j, :j] * x[j]
    return x


def compose(T_icp, n):
    """The reference's full_registration from the n (n - 1) / 2 ICPs in its loop order: a graph of the oracle."""
    edges = [(s, t) for s in range(n) for t in range(s + 1, n)]
    odometry, nodes = np.eye(4), [np.eye(4)]
    for k in range(1, n):
        odometry = T_icp[edges.index((k - 1, k))] @ odometry
        nodes.append(rigid_inv(odometry))
    return {"nodes": np.stack(nodes), "edges": edges, "T": np.asarray(T_icp), "uncertain": [t != s + 1 for s, t in edges]}


class _Margins(dict):
    def see(self, kind, a, b):
        a, b = float(a), float(b)
        m = abs(a - b) / max(abs(a), abs(b), 1e-300)
        self[kind] = min(self.get(kind, np.inf), m)


def _mat2vec(M, margins):
    dt = M.dtype.type
    sy = np.hypot(M[0, 0], M[1, 0])
    margins.see("sy", sy, 1e-6)
    if sy > dt(1e-6):
        v = [np.arctan2(M[2, 1], M[2, 2]), np.arctan2(-M[2, 0], sy), np.arctan2(M[1, 0], M[0, 0])]
    else:
        v = [np.arctan2(-M[1, 2], M[1, 1]), np.arctan2(-M[2, 0], sy), dt(0)]
    return np.array(v + [M[0, 3], M[1, 3], M[2, 3]], dtype=M.dtype)


class _Pass:
    def __init__(self, g, T, conf, active, option, criteria, dt, margins):
        self.g, self.T, self.conf, self.active, self.o, self.c, self.dt, self.m = g, T, conf, active, option, criteria, dt, margins
        self.gen = _generators(dt)
        self.N = 6 * len(T)

    def errors(self, T):
        g = self.g
        e = np.zeros((len(g["edges"]), 6), dtype=self.dt)
        r = np.zeros(len(g["edges"]), dtype=self.dt)
        for k, (s, t) in enumerate(g["edges"]):
            if self.active[k]:
                e[k] = lin6(g["Xinv"][k] @ rigid_inv(T[t]) @ T[s])
                r[k] = e[k] @ (g["info"][k] @ e[k])
        return e, r

    def residual(self, r, w):
        s = self.dt(0)
        for k in range(len(r)):
            if self.active[k]:
                s += self.conf[k] * r[k] + w * (np.sqrt(self.conf[k]) - 1) ** 2
        return s

    def update_confidence(self, r, w):
        for k in range(len(r)):
            if self.active[k] and self.g["uncertain"][k]:
                self.conf[k] = (w / (w + r[k])) ** 2

    def linear_system(self, T, e):
        g = self.g
        H = np.zeros((self.N, self.N), dtype=self.dt)
        b = np.zeros(self.N, dtype=self.dt)
        for k, (s, t) in enumerate(g["edges"]):
            if not self.active[k]:
                continue
            P = g["Xinv"][k] @ rigid_inv(T[t])
            J = np.stack([lin6(P @ (self.gen[i] @ T[s])) for i in range(6)], axis=1)
            I, c = g["info"][k], self.conf[k]
            A, gv = J.T @ (I @ J), J.T @ (I @ e[k])
            S, D = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
            H[S, S] += c * A
            H[S, D] -= c * A
            H[D, S] -= c * A
            H[D, D] += c * A
            b[S] -= c * gv
            b[D] += c * gv
        return H, b

    def run(self):
        c, dt, m = self.c, self.dt, self.m
        act = [k for k in range(len(self.active)) if self.active[k]]
        if not act:
            return 1, 0, dt(0)
        w = dt(self.o["preference_loop_closure"]) * dt(self.o["max_correspondence_distance"]) ** 2 * \
            (sum((self.g["info"][k][5, 5] for k in act), dt(0)) / dt(len(act)))
        if not w > 0:
            return 1, 0, dt(0)
        T = self.T
        e, r = self.errors(T)
        residual = self.residual(r, w)
        self.update_confidence(r, w)
        H, b = self.linear_system(T, e)
        lam, nu = dt(1e-5) * H.diagonal().max(), dt(2)
        x = np.concatenate([_mat2vec(Ti, m) for Ti in T])
        solves = 0
        m.see("right_term", b.max(), c["min_right_term"])
        if b.max() < dt(c["min_right_term"]):
            return 0, solves, residual
        stop, it = False, 0
        while not stop:
            trials, rho = 0, dt(0)
            while True:
                delta = ldlt_solve(H + lam * np.eye(self.N, dtype=dt), b)
                if delta is None:
                    return 3, solves, residual
                solves += 1
                nd = np.sqrt((delta * delta).sum())
                lim = dt(c["min_relative_increment"]) * (np.sqrt((x * x).sum()) + dt(c["min_relative_increment"]))
                m.see("increment", nd, lim)
                if nd < lim:
                    stop = True
                else:
                    Tn = np.stack([vec2mat(delta[6 * i:6 * i + 6]) @ T[i] for i in range(len(T))])
                    en, rn = self.errors(Tn)
                    fresh = self.residual(rn, w)
                    m.see("descent", fresh, residual)
                    rho = (residual - fresh) / ((delta * (lam * delta + b)).sum() + dt(1e-3))
                    if rho > 0:
                        m.see("residual_increment", residual - fresh, dt(c["min_relative_residual_increment"]) * residual)
                        if residual - fresh < dt(c["min_relative_residual_increment"]) * residual:
                            stop = True
                            break
                        alpha = dt(1) - (dt(2) * rho - dt(1)) ** 3
                        lam = lam * max(dt(c["lower_scale_factor"]), min(alpha, dt(c["upper_scale_factor"])))
                        nu = dt(2)
                        residual, T, e, r = fresh, Tn, en, rn
                        x = np.concatenate([_mat2vec(Ti, m) for Ti in T])
                        self.update_confidence(r, w)
                        H, b = self.linear_system(T, e)
                        m.see("right_term", b.max(), c["min_right_term"])
                        if b.max() < dt(c["min_right_term"]):
                            stop = True
                            break
                    else:
                        lam, nu = lam * nu, nu * 2
                trials += 1
                stop = stop or trials >= c["max_iteration_lm"]
                if rho > 0 or stop:
                    break
            m.see("min_residual", residual, c["min_residual"])
            stop = stop or residual < dt(c["min_residual"]) or it >= c["max_iteration"]
            it += 1
        self.T = T
        return 0, solves, residual


def global_optimization(graph, max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0,
                        reference_node=0, criteria=None, dtype=np.float64):
    dt = np.dtype(dtype).type
    c = dict(DEFAULT_CRITERIA, **(criteria or {}))
    o = dict(max_correspondence_distance=max_correspondence_distance, preference_loop_closure=preference_loop_closure)
    nodes = np.asarray(graph["nodes"], dtype=np.float64)
    n, m = len(nodes), len(graph["edges"])
    out = {"poses": nodes.astype(dt), "confidence": np.ones(m, dtype=dt), "kept": np.ones(m, dtype=np.int32), "solves": (0, 0),
           "residual": dt(0), "status": 0, "margins": _Margins()}
    if not (np.isfinite(nodes).all() and np.isfinite(np.asarray(graph["T"], dtype=np.float64)).all()
            and np.isfinite(np.asarray(graph["info"], dtype=np.float64)).all()):
        out["status"] = 2
        return out
    g = {"edges": [(int(s), int(t)) for s, t in graph["edges"]], "uncertain": [bool(u) for u in graph["uncertain"]],
         "info": np.asarray(graph["info"], dtype=np.float64).astype(dt).reshape(m, 6, 6),
         "Xinv": np.stack([rigid_inv(X) for X in np.asarray(graph["T"], dtype=np.float64).astype(dt).reshape(m, 4, 4)])}
    conf, active, margins = np.ones(m, dtype=dt), np.ones(m, dtype=bool), out["margins"]
    p1 = _Pass(g, nodes.astype(dt), conf, active, o, c, dt, margins)
    st, s1, res = p1.run()
    s2 = 0
    if st == 0:
        for k in range(m):
            if g["uncertain"][k]:
                margins.see("prune", conf[k], edge_prune_threshold)
        active = np.array([(not g["uncertain"][k]) or conf[k] > dt(edge_prune_threshold) for k in range(m)])
        p2 = _Pass(g, p1.T, conf, active, o, c, dt, margins)
        st, s2, res = p2.run()
        if st == 0:
            F = nodes[reference_node].astype(dt) @ rigid_inv(p2.T[reference_node])
            out.update(poses=np.stack([F @ Ti for Ti in p2.T]), confidence=conf, kept=active.astype(np.int32),
                       solves=(s1, s2), residual=res)
    out["status"] = st
    return out
