"""NumPy restatement of the Levenberg-Marquardt pose refinement of csrc/pnp.hip (lm_refine, scpose_pnp_epnp_ransac_refine).

Test infrastructure, not product and not an oracle of cv2: the kernel restates cv2.solvePnPRefineLM from OpenCV's documentation
(unpinned against cv2, like oracle/pnp_ref.c), and this file restates the kernel's algorithm step for step so that the GPU tests
can pin it -- parametrisation, damping schedule, stop rule -- while tests/pnp_independent.py (SciPy) pins the answer it converges to.

  * parameters p = (rvec, tvec); R = Rodrigues(rvec) computed as the kernel's rodrigues_vec2mat does;
  * residuals: project_point (pinhole + k1, k2, p1, p2, k3) of the landmark, rounded through float32 as the kernel's LDS copy
    is, minus the raw float32 image point; cost = sum of squared residuals;
  * analytic Jacobian: d(R X)/d rvec = -[R X]x (r r^T + [r]x (I - R)) / theta^2 (-[X]x below theta = DBL_EPSILON), through
    the perspective division and the distortion model;
  * step: Cholesky solve of (A + lambda diag(A)) d = -g with A = J^T J, g = J^T r; a matrix that is not positive definite counts
    as a rejected step; accept when the cost strictly drops (lambda / 10), else reject (lambda * 10); lambda_0 = 1e-3; stop after
    `iters` iterations, or after the iteration whose step had |d| <= FLT_EPSILON |p| (taken if it lowered the cost).
The only differences from the kernel are summation orders (the kernel sums over points with a lane butterfly), so results
agree to rounding, not bit for bit.
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)


def rodrigues(r):
    theta = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta < DBL_EPSILON:
        return np.eye(3)
    c, s = np.cos(theta), np.sin(theta)
    rx, ry, rz = r / theta
    rrt = np.array([[rx * rx, rx * ry, rx * rz], [rx * ry, ry * ry, ry * rz], [rx * rz, ry * rz, rz * rz]])
    rxm = np.array([[0, -rz, ry], [rz, 0, -rx], [-ry, rx, 0]])
    return (1 - c) * rrt + s * rxm + c * np.eye(3)


def residuals_jacobian(p, X, uv, K, dist):
    """Residuals (m, 2) and Jacobian (m, 2, 6) at p."""
    r, t = p[:3], p[3:]
    R = rodrigues(r)
    Y = X @ R.T
    th2 = float(r @ r)
    if np.sqrt(th2) >= DBL_EPSILON:
        S = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        M = (np.outer(r, r) + S @ (np.eye(3) - R)) / th2
    else:
        M = np.eye(3)
    Yx = np.zeros((len(X), 3, 3))
    Yx[:, 0, 1], Yx[:, 0, 2], Yx[:, 1, 2] = -Y[:, 2], Y[:, 1], -Y[:, 0]
    Yx[:, 1, 0], Yx[:, 2, 0], Yx[:, 2, 1] = Y[:, 2], -Y[:, 1], Y[:, 0]
    dY = -Yx @ M                                               # (m, 3, 3): d Y / d rvec
    Pc = Y + t
    iz = 1.0 / Pc[:, 2]
    x, y = Pc[:, 0] * iz, Pc[:, 1] * iz
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    cdist = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    dc = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2
    xd = x * cdist + p1 * 2 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cdist + p1 * (r2 + 2 * y * y) + p2 * 2 * x * y
    res = np.stack([xd * K[0, 0] + K[0, 2] - uv[:, 0], yd * K[1, 1] + K[1, 2] - uv[:, 1]], 1)
    dxx = cdist + 2 * x * x * dc + 2 * p1 * y + 6 * p2 * x
    dxy = 2 * x * y * dc + 2 * p1 * x + 2 * p2 * y
    dyy = cdist + 2 * y * y * dc + 6 * p1 * y + 2 * p2 * x
    du = K[0, 0] * np.stack([dxx * iz, dxy * iz, -(dxx * x + dxy * y) * iz], 1)        # (m, 3): d u / d Pc
    dv = K[1, 1] * np.stack([dxy * iz, dyy * iz, -(dxy * x + dyy * y) * iz], 1)
    J = np.zeros((len(X), 2, 6))
    J[:, 0, :3] = np.einsum("mi,mij->mj", du, dY)
    J[:, 1, :3] = np.einsum("mi,mij->mj", dv, dY)
    J[:, 0, 3:], J[:, 1, 3:] = du, dv
    return res, J


def cost(p, X, uv, K, dist):
    res, _ = residuals_jacobian(p, X, uv, K, dist)
    return float((res * res).sum())


def _solve(A, g, lam):
    """Cholesky solve of (A + lam diag(A)) d = -g, None when not positive definite (the kernel's lm_solve)."""
    B = A.copy()
    B[np.diag_indices(6)] += lam * np.diag(A)
    L = np.zeros((6, 6))
    for j in range(6):
        s = B[j, j] - L[j, :j] @ L[j, :j]
        if not s > 0:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (B[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - L[i, :i] @ y[:i]) / L[i, i]
    d = np.zeros(6)
    for i in range(5, -1, -1):
        d[i] = (y[i] - L[i + 1:, i] @ d[i + 1:]) / L[i, i]
    return d


def refine(rvec, tvec, X, uv, K, dist, iters=20, trace=None, eps=FLT_EPSILON):
    """The kernel's lm_refine.  X: landmarks of the final point set (rounded through float32 here), uv: their raw float32
    image points.  Returns (rvec, tvec); `trace`, when a list, receives the cost after every iteration.  eps is the kernel's
    FLT_EPSILON; eps = 0 runs the whole budget (tests use it to reach the fixed point itself)."""
    X = np.asarray(X, dtype=np.float64).astype(np.float32).astype(np.float64)
    uv = np.asarray(uv, dtype=np.float32).astype(np.float64)
    K = np.asarray(K, dtype=np.float64); dist = np.asarray(dist, dtype=np.float64)
    p0 = np.concatenate([np.asarray(rvec, dtype=np.float64), np.asarray(tvec, dtype=np.float64)])
    p = p0.copy()
    res, J = residuals_jacobian(p, X, uv, K, dist)
    c = float((res * res).sum())
    A = np.einsum("mki,mkj->ij", J, J)
    g = np.einsum("mki,mk->i", J, res)
    lam = 1e-3
    for _ in range(iters):
        d = _solve(A, g, lam)
        if d is None:
            lam *= 10
            if trace is not None:
                trace.append(c)
            continue
        converged = np.sqrt(d @ d) <= eps * np.sqrt(p @ p)
        q = p + d
        res, J = residuals_jacobian(q, X, uv, K, dist)
        cq = float((res * res).sum())
        if cq < c:
            p, c = q, cq
            A = np.einsum("mki,mkj->ij", J, J)
            g = np.einsum("mki,mk->i", J, res)
            lam /= 10
        else:
            lam *= 10
        if trace is not None:
            trace.append(c)
        if converged:
            break
    if not np.all(np.isfinite(p)):
        p = p0
    return p[:3], p[3:]
