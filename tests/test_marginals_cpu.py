"""movba_lba_marginals without a GPU: the C-ABI's new entry point and status, and the numpy reference that the GPU tests
(test_gpu_marginals.py) hold the device to, checked against itself.

The reference restates the normal matrix of tests/golden/make_golden.py's lm_dense loop (every edge, Huber weight
rho'(chi2) inv_sigma2, stereo third rows, cameras by keyframe) at a given estimate, plus `damping` on the diagonal, in two
forms: the full (6 K + 3 P) matrix, inverted with numpy.linalg.inv, and the Schur form the library computes (S = Hpp - Hpl
Hll^-1 Hlp; pose block (S^-1)_ii, point block D + D (Hpl^T S^-1 Hpl)_ll D).  Both must give the same blocks."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import make_golden as mg  # noqa: E402


def edge_terms(w, poses, points):
    """Per edge at (poses, points): point Jacobian rows A (E, 3, 3), pose Jacobian rows B (E, 3, 6) over the left tangent
    [omega; upsilon] of Tcw (expm(twist(dx)) @ T, as lm_dense updates), weight om = rho'(chi2) inv_sigma2 (E,).  Third rows
    are zero for monocular edges.  The same expressions as make_golden.lm_dense, for all edges at once."""
    Ts = np.stack([mg.T_from_qt(q) for q in np.asarray(poses, np.float64)])
    X = np.asarray(points, np.float64)
    e, Xc = mg.errors(Ts, X, w)
    fx, fy, _, _, bf = mg.edge_cameras(w)
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    E = w.n_edges
    Jpi = np.zeros((E, 3, 3))
    Jpi[:, 0, 0] = fx / z; Jpi[:, 0, 2] = -fx * x / z ** 2
    Jpi[:, 1, 1] = fy / z; Jpi[:, 1, 2] = -fy * y / z ** 2
    if w.obs_right is not None:
        st = np.asarray(w.obs_right) >= 0
        Jpi[st, 2, 0] = fx[st] / z[st]; Jpi[st, 2, 2] = -fx[st] * x[st] / z[st] ** 2 + bf[st] / z[st] ** 2
    R = Ts[w.edge_pose][:, :3, :3]
    A = -Jpi @ R
    skew = np.zeros((E, 3, 3))
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 2] = -z, y, -x
    skew[:, 1, 0], skew[:, 2, 0], skew[:, 2, 1] = z, -y, x
    B = -Jpi @ np.concatenate([-skew, np.broadcast_to(np.eye(3), (E, 3, 3))], axis=2)
    chi2 = w.inv_sigma2 * (e ** 2).sum(1)
    wgt = np.array([mg.huber(c, w.huber_delta)[1] for c in chi2]) if E else np.zeros(0)
    return A, B, wgt * w.inv_sigma2


def hessian_index(w):
    """hessian index of every keyframe: free keyframes WITH an edge, in caller order (-1: fixed or without an edge)"""
    has = np.zeros(w.n_poses, bool)
    has[w.edge_pose] = True
    act = (np.asarray(w.pose_fixed) == 0) & has
    hidx = -np.ones(w.n_poses, int)
    hidx[act] = np.arange(act.sum())
    return hidx, int(act.sum())


def full_hessian(w, poses, points, damping=0.0):
    """The full normal matrix (6 nfree + 3 P square) at (poses, points) with `damping` on its diagonal: make_golden.lm_dense's
    loop.  -> (H, hidx, nfree)"""
    A, B, om = edge_terms(w, poses, points)
    hidx, nf = hessian_index(w)
    P = w.n_points
    off = 6 * nf
    H = np.zeros((off + 3 * P, off + 3 * P))
    for k in range(w.n_edges):
        ip, l = w.edge_pose[k], w.edge_point[k]
        sl = slice(off + 3 * l, off + 3 * l + 3)
        H[sl, sl] += om[k] * A[k].T @ A[k]
        if hidx[ip] >= 0:
            sp = slice(6 * hidx[ip], 6 * hidx[ip] + 6)
            H[sp, sp] += om[k] * B[k].T @ B[k]
            H[sp, sl] += om[k] * B[k].T @ A[k]; H[sl, sp] += om[k] * A[k].T @ B[k]
    H[np.diag_indices_from(H)] += damping
    return H, hidx, nf


def _blocks_from_inverse(w, Hinv, hidx, nf):
    pose = np.full((w.n_poses, 6, 6), np.nan)
    pose[np.asarray(w.pose_fixed) != 0] = 0.0
    for i in np.flatnonzero(hidx >= 0):
        h = hidx[i]
        pose[i] = Hinv[6 * h:6 * h + 6, 6 * h:6 * h + 6]
    off = 6 * nf
    pts = np.stack([Hinv[off + 3 * l:off + 3 * l + 3, off + 3 * l:off + 3 * l + 3] for l in range(w.n_points)])
    return pose, pts


def marginals_full(w, poses, points, damping=0.0):
    """The blocks of inv(H) of the full matrix: (pose_cov (NP, 6, 6), point_cov (P, 3, 3))"""
    H, hidx, nf = full_hessian(w, poses, points, damping)
    return _blocks_from_inverse(w, np.linalg.inv(H), hidx, nf)


def marginals_schur(w, poses, points, damping=0.0):
    """The blocks in the Schur form the library defines (include/movba.h): -> dict(pose_cov, point_cov, cond_S).  Fixed
    keyframes get zero blocks, free keyframes and points without an edge NaN."""
    A, B, om = edge_terms(w, poses, points)
    hidx, nf = hessian_index(w)
    P, E = w.n_points, w.n_edges
    ep, el = np.asarray(w.edge_pose), np.asarray(w.edge_point)
    Hll = np.zeros((P, 3, 3))
    np.add.at(Hll, el, om[:, None, None] * np.einsum("eki,ekj->eij", A, A))
    Hll += damping * np.eye(3)
    has_pt = np.zeros(P, bool)
    has_pt[el] = True
    D = np.full((P, 3, 3), np.nan)
    D[has_pt] = np.linalg.inv(Hll[has_pt])
    fe = hidx[ep] >= 0                                              # edges of free keyframes
    h = hidx[ep[fe]]
    Hpp = np.zeros((nf, 6, nf, 6))
    np.add.at(Hpp, (h, slice(None), h), om[fe, None, None] * np.einsum("eki,ekj->eij", B[fe], B[fe]))
    Hpp = Hpp.reshape(6 * nf, 6 * nf) + damping * np.eye(6 * nf)
    Hpl = np.zeros((nf, 6, P, 3))                                   # one block per edge: a keyframe observes a point once
    np.add.at(Hpl, (h, slice(None), el[fe]), om[fe, None, None] * np.einsum("eki,ekj->eij", B[fe], A[fe]))
    Hpl = Hpl.reshape(6 * nf, P, 3)
    Dz = np.where(has_pt[:, None, None], D, 0.0)
    HplD = np.einsum("npi,pij->npj", Hpl, Dz)
    S = Hpp - HplD.reshape(6 * nf, 3 * P) @ Hpl.reshape(6 * nf, 3 * P).T
    Sig = np.linalg.inv(S)
    pose = np.full((w.n_poses, 6, 6), np.nan)
    pose[np.asarray(w.pose_fixed) != 0] = 0.0
    for i in np.flatnonzero(hidx >= 0):
        k = hidx[i]
        pose[i] = Sig[6 * k:6 * k + 6, 6 * k:6 * k + 6]
    Y = (Sig @ Hpl.reshape(6 * nf, 3 * P)).reshape(6 * nf, P, 3)
    M = np.einsum("npi,npj->pij", Hpl, Y)                           # sum_ij B_il^T Sigma_ij B_jl
    pts = D + D @ M @ D
    return dict(pose_cov=pose, point_cov=pts, cond_S=float(np.linalg.cond(S)), S=S)


def rel_block_err(got, want):
    """largest relative Frobenius error over the blocks that are finite and non-zero in `want`"""
    g = got.reshape(len(got), -1); r = want.reshape(len(want), -1)
    ok = np.isfinite(r).all(1) & (np.abs(r).sum(1) > 0)
    if not ok.any():
        return 0.0
    return float((np.linalg.norm(g[ok] - r[ok], axis=1) / np.linalg.norm(r[ok], axis=1)).max())


# golden windows at their golden outputs; tiny and norobust are monocular with one fixed keyframe (free scale): damped
CASES = [("small", 0.0), ("hard", 0.0), ("stereo", 0.0), ("cameras", 0.0), ("tiny", 1e-3), ("norobust", 1e-3)]


@pytest.mark.parametrize("name,damping", CASES)
def test_reference_schur_form_equals_the_inverse_of_the_full_matrix(name, damping):
    w, out = load_golden("lba_" + name)
    full_pose, full_pts = marginals_full(w, out["poses"], out["points"], damping)
    ref = marginals_schur(w, out["poses"], out["points"], damping)
    print(f"{name}: damping {damping:g}, cond(S) {ref['cond_S']:.3g}")
    assert ref["cond_S"] < 1e7
    assert rel_block_err(ref["pose_cov"], full_pose) < 1e-9
    assert rel_block_err(ref["point_cov"], full_pts) < 1e-9
    fixed = np.asarray(w.pose_fixed) != 0
    assert np.all(ref["pose_cov"][fixed] == 0) and np.isfinite(ref["pose_cov"][~fixed]).all()
    for blk in list(ref["pose_cov"][~fixed]) + list(ref["point_cov"]):
        np.linalg.cholesky(0.5 * (blk + blk.T))


def test_reference_sees_the_free_scale_of_undamped_monocular_windows():
    """tiny / norobust: one fixed keyframe, monocular - the scale is a gauge freedom, S is numerically singular undamped"""
    for name in ("tiny", "norobust"):
        w, out = load_golden("lba_" + name)
        assert int(np.asarray(w.pose_fixed).sum()) == 1 and w.obs_right is None
        c0 = marginals_schur(w, out["poses"], out["points"], 0.0)["cond_S"]
        c1 = marginals_schur(w, out["poses"], out["points"], 1e-3)["cond_S"]
        assert c0 > 1e12 and c1 < 1e7, (name, c0, c1)


def test_library_exports_marginals_and_solver_has_it(built_lib):
    lib = built_lib.lib()
    assert hasattr(lib, "movba_lba_marginals")
    assert hasattr(built_lib.lib(hooks=True), "movba_lba_marginals")
    assert "movba_lba_marginals" in built_lib.EXPORTS
    assert callable(getattr(built_lib.Solver, "marginals", None))
    assert built_lib.SINGULAR == 4


def test_null_handle_and_bad_arguments_are_refused(built_lib):
    import ctypes as C
    lib = built_lib.lib()
    buf = (C.c_double * 36)()
    p = C.cast(buf, C.POINTER(C.c_double))
    assert lib.movba_lba_marginals(None, 0.0, p, None) == built_lib.ERR_ARG
    assert lib.movba_lba_marginals(None, 0.0, None, p) == built_lib.ERR_ARG
    assert lib.movba_lba_marginals(None, 0.0, None, None) == built_lib.ERR_ARG
    assert all(v == 0.0 for v in buf)


def test_status_string_names_the_singular_case(built_lib):
    assert "singular" in built_lib.status_string(built_lib.SINGULAR)
    assert built_lib.status_string(3) == "nothing to optimise" and built_lib.status_string(5) == "unknown"


def test_header_documents_the_new_status_and_definition():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "movba.h")).read()
    assert "#define MOVBA_SINGULAR        4" in hdr
    decl = hdr[hdr.index("int  movba_lba_marginals"):]
    assert decl.startswith("int  movba_lba_marginals(movba_handle *h, double damping, double *pose_cov, double *point_cov);")
