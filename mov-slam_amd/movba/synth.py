"""Seeded synthetic covisibility windows (BASELINE.md cfg 1-3, 5).

The generator stands in for the graph `Optimizer::LocalBundleAdjustment` builds at
/root/reference/src/Optimizer.cc:464-747: K free + F fixed keyframe vertices, P map
points, one monocular edge per (point, observing keyframe), pinhole fx=fy=320,
cx=320, cy=240 on 640x480 (Examples/Monocular/TartanAir.yaml:15-26).  All values are
rounded to float32 and widened, mimicking the float->double casts at
Optimizer.cc:559, 627, 650.  Edge order: point id ascending, then keyframe id
ascending (stands in for the reference's std::map<KeyFrame*> pointer order).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

FX = FY = 320.0
CX, CY = 320.0, 240.0
WIDTH, HEIGHT = 640, 480
HUBER_DELTA = float(np.sqrt(np.float32(5.0)))  # (double)sqrtf(5.0f): Optimizer.cc:616
CHI2_GATE = 5.0                                   # static float delta, Optimizer.cc:52, 769


@dataclass
class Window:
    """Flattened local-BA window in the layout the C-ABI takes (include/movba.h)."""
    poses: np.ndarray        # (NP,7) f64  qx qy qz qw tx ty tz (Tcw), ascending keyframe id
    pose_fixed: np.ndarray   # (NP,)  u8
    points: np.ndarray       # (P,3)  f64
    edge_pose: np.ndarray    # (E,)   i32
    edge_point: np.ndarray   # (E,)   i32
    obs: np.ndarray          # (E,2)  f64
    inv_sigma2: np.ndarray   # (E,)   f64
    cam: tuple = (FX, FY, CX, CY)
    huber_delta: float = HUBER_DELTA
    chi2_gate: float = CHI2_GATE
    max_iters: int = 10
    truth_poses: np.ndarray | None = None
    truth_points: np.ndarray | None = None
    meta: dict = field(default_factory=dict)
    obs_right: np.ndarray | None = None   # (E,) f64: right-image u of stereo observations, < 0 = monocular edge
    bf: float = 0.0                       # KeyFrame::mbf (baseline * fx)
    cam_kf: np.ndarray | None = None      # (NP,4) f64: fx fy cx cy by keyframe (None: `cam` for all, every shipped configuration)
    bf_kf: np.ndarray | None = None       # (NP,)  f64: mbf by keyframe

    @property
    def n_poses(self): return int(self.poses.shape[0])
    @property
    def n_free(self): return int((self.pose_fixed == 0).sum())
    @property
    def n_points(self): return int(self.points.shape[0])
    @property
    def n_edges(self): return int(self.edge_pose.shape[0])


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def quat_from_R(R):
    """Rotation matrix -> unit quaternion (x,y,z,w), w >= 0."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[i] = 0.25 * s
        q[3] = (R[k, j] - R[j, k]) / s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def R_from_quat(q):
    x, y, z, w = q
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def make_window(n_free: int, n_fixed: int, n_points: int, seed: int,
                run_lo: int = 2, run_hi: int = 10, outlier_frac: float = 0.05,
                pix_sigma: float = 0.5, rot_sigma_deg: float = 0.5, trans_sigma: float = 0.02,
                point_sigma: float = 0.05, min_obs: int = 2, stereo_frac: float = 0.0, bf: float = 80.0) -> Window:
    rng = np.random.default_rng(seed)
    NP = n_free + n_fixed
    k = np.arange(NP, dtype=np.float64)
    centres = np.stack([0.30 * k, 0.05 * np.sin(0.3 * k), 0.02 * k], axis=1)
    yaw = 0.01 * k
    Rcw = np.zeros((NP, 3, 3))
    tcw = np.zeros((NP, 3))
    for i in range(NP):
        c, s = np.cos(yaw[i]), np.sin(yaw[i])
        Rwc = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])   # yaw about the camera's y axis
        Rcw[i] = Rwc.T
        tcw[i] = -Rcw[i] @ centres[i]

    # candidate points until P of them have >= min_obs valid observations
    pts, e_pose, e_point, e_uv = [], [], [], []
    n_kept = 0
    while n_kept < n_points:
        m = max(256, (n_points - n_kept) * 2)
        anchor = rng.integers(0, NP, size=m)
        depth = rng.uniform(4.0, 30.0, size=m)
        u = rng.uniform(0.0, WIDTH, size=m)
        v = rng.uniform(0.0, HEIGHT, size=m)
        run = rng.integers(run_lo, run_hi + 1, size=m)
        off = rng.integers(0, run_hi + 1, size=m)
        for j in range(m):
            if n_kept >= n_points:
                break
            a = int(anchor[j])
            Xc = np.array([(u[j] - CX) / FX * depth[j], (v[j] - CY) / FY * depth[j], depth[j]])
            Xw = Rcw[a].T @ (Xc - tcw[a])
            first = a - int(off[j]) % int(run[j])
            ks = [kk for kk in range(first, first + int(run[j])) if 0 <= kk < NP]
            uv_ok = []
            for kk in ks:
                Y = Rcw[kk] @ Xw + tcw[kk]
                if Y[2] <= 0.1:
                    continue
                uu, vv = FX * Y[0] / Y[2] + CX, FY * Y[1] / Y[2] + CY
                if 0 <= uu < WIDTH and 0 <= vv < HEIGHT:
                    uv_ok.append((kk, uu, vv))
            if len(uv_ok) < min_obs:
                continue
            pts.append(Xw)
            for kk, uu, vv in uv_ok:
                e_pose.append(kk); e_point.append(n_kept); e_uv.append((uu, vv))
            n_kept += 1

    truth_points = np.array(pts)
    edge_pose = np.array(e_pose, dtype=np.int32)
    edge_point = np.array(e_point, dtype=np.int32)
    obs = np.array(e_uv, dtype=np.float64)
    E = len(edge_pose)
    obs = obs + rng.normal(0.0, pix_sigma, size=(E, 2))
    is_out = rng.random(E) < outlier_frac
    mag = rng.uniform(5.0, 30.0, size=E)
    ang = rng.uniform(0.0, 2 * np.pi, size=E)
    obs[is_out] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)[is_out]

    # stereo observations (Optimizer.cc:673-705): u_right = u - bf / z (+ noise) for a fraction of the edges
    obs_right = None
    if stereo_frac > 0.0:
        Xc_all = np.einsum('eij,ej->ei', Rcw[edge_pose], truth_points[edge_point]) + tcw[edge_pose]
        ur = obs[:, 0] - bf / Xc_all[:, 2] + rng.normal(0.0, pix_sigma, size=E)
        st = (rng.random(E) < stereo_frac) & (ur >= 0.0)
        obs_right = np.where(st, ur, -1.0)

    truth_poses = np.zeros((NP, 7))
    poses = np.zeros((NP, 7))
    fixed = np.zeros(NP, dtype=np.uint8)
    fixed[:n_fixed] = 1                                     # the F lowest-id keyframes, exact truth
    for i in range(NP):
        truth_poses[i, :4] = quat_from_R(Rcw[i]); truth_poses[i, 4:] = tcw[i]
        if fixed[i]:
            poses[i] = truth_poses[i]
        else:
            dR = _rodrigues(np.deg2rad(rot_sigma_deg) * rng.normal(size=3))
            poses[i, :4] = quat_from_R(dR @ Rcw[i])
            poses[i, 4:] = tcw[i] + trans_sigma * rng.normal(size=3)
    points = truth_points + point_sigma * rng.normal(size=truth_points.shape)

    poses = _f32(poses)
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)   # cast<double> of a unit float quat, renormalised by SE3Quat
    return Window(poses=poses, pose_fixed=fixed, points=_f32(points), edge_pose=edge_pose,
                  edge_point=edge_point, obs=_f32(obs), inv_sigma2=np.ones(E),
                  truth_poses=truth_poses, truth_points=truth_points,
                  meta=dict(seed=seed, K=n_free, F=n_fixed, P=n_points, E=E, outliers=int(is_out.sum())),
                  obs_right=None if obs_right is None else np.where(obs_right >= 0, _f32(obs_right), -1.0), bf=bf if obs_right is not None else 0.0)


def cfg(name: str, seed: int | None = None) -> Window:
    """Named BASELINE.md configurations."""
    if name == "tiny":      # golden-fixture size (3 KF x 20 points)
        return make_window(2, 1, 20, 7 if seed is None else seed, run_lo=2, run_hi=3)
    if name == "small":     # golden-fixture size (10 KF x 200 points)
        return make_window(8, 2, 200, 11 if seed is None else seed, run_lo=2, run_hi=6)
    if name == "cfg2":      # LBA 10 KF x 2k MapPoints
        return make_window(10, 2, 2000, 1002 if seed is None else seed, run_lo=2, run_hi=6)
    if name == "cfg3":      # LBA 50 KF x 20k MapPoints, Huber on
        return make_window(50, 10, 20000, 1003 if seed is None else seed, run_lo=2, run_hi=10)
    raise KeyError(name)


def make_frame(n: int = 500, seed: int = 1001, outlier_frac: float = 0.10, pix_sigma: float = 0.5):
    """cfg1: one Frame with n 2D-3D matches (PoseOptimization operand, Optimizer.cc:404-413)."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(4.0, 30.0, size=n)
    u = rng.uniform(0, WIDTH, size=n); v = rng.uniform(0, HEIGHT, size=n)
    Xc = np.stack([(u - CX) / FX * depth, (v - CY) / FY * depth, depth], axis=1)
    Rcw = _rodrigues(np.array([0.02, -0.03, 0.01])); tcw = np.array([0.3, -0.1, 0.2])
    Xw = (Xc - tcw) @ Rcw                                    # Rcw^T (Xc - t)
    obs = np.stack([u, v], axis=1) + rng.normal(0, pix_sigma, size=(n, 2))
    is_out = rng.random(n) < outlier_frac
    mag = rng.uniform(10.0, 60.0, size=n); ang = rng.uniform(0, 2 * np.pi, size=n)
    obs[is_out] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)[is_out]
    truth = np.concatenate([quat_from_R(Rcw), tcw])
    dR = _rodrigues(np.deg2rad(1.0) * rng.normal(size=3))
    pose0 = np.concatenate([quat_from_R(dR @ Rcw), tcw + 0.05 * rng.normal(size=3)])
    pose0 = _f32(pose0); pose0[:4] /= np.linalg.norm(pose0[:4])
    return dict(Xw=_f32(Xw), obs=_f32(obs), pose0=pose0, truth=truth, is_outlier=is_out,
                cam=(FX, FY, CX, CY))


# ---------------------------------------------------------------------------------------------
# Covisibility patterns beyond the contiguous-run generator above (round 3).
#
# make_window() gives every map point a contiguous run of observing keyframes, and keyframe ids follow the
# trajectory: the reduced system is banded.  The reference's local window is "every keyframe sharing >= 15 points
# with pKF" (/root/reference/src/KeyFrame.cc:227-231, 408-427; selection src/Optimizer.cc:464-477): all of them
# covisible through pKF and mostly with each other, ids in order of creation, not of position.  The patterns below
# produce such windows with consistent geometry (every observation is the projection of its map point):
#   hub      keyframes clustered around one place, all looking at the same scene: every pair shares points,
#   revisit  the trajectory comes back over itself: keyframe k and k + 25 see the same points,
#   shuffle_ids()  any window with its keyframe ids permuted (same graph, id order != spatial order).
# ---------------------------------------------------------------------------------------------
def _poses_from(centres, yaw):
    NP = len(yaw)
    Rcw = np.zeros((NP, 3, 3)); tcw = np.zeros((NP, 3))
    for i in range(NP):
        c, s = np.cos(yaw[i]), np.sin(yaw[i])
        Rwc = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        Rcw[i] = Rwc.T
        tcw[i] = -Rcw[i] @ centres[i]
    return Rcw, tcw


def make_pattern_window(pattern: str, n_free: int, n_fixed: int, n_points: int, seed: int,
                        run_lo: int = 2, run_hi: int = 10, outlier_frac: float = 0.05, pix_sigma: float = 0.5,
                        rot_sigma_deg: float = 0.5, trans_sigma: float = 0.02, point_sigma: float = 0.05,
                        min_obs: int = 2, revisit_gap: int = 25) -> Window:
    """Window with the covisibility pattern `pattern` ("hub" | "revisit"); noise model, camera, float32 rounding, edge order
    and the choice of fixed keyframes (the n_fixed lowest ids) as make_window()."""
    rng = np.random.default_rng(seed)
    NP = n_free + n_fixed
    k = np.arange(NP, dtype=np.float64)
    if pattern == "hub":
        centres = np.stack([rng.uniform(-1.5, 1.5, NP), rng.uniform(-0.3, 0.3, NP), rng.uniform(-1.0, 1.0, NP)], axis=1)
        yaw = rng.uniform(-0.15, 0.15, NP)
        order_key = None
    elif pattern == "revisit":
        # second pass over the same stretch of path, half a keyframe spacing out of step and 0.2 m to the side
        first = NP - revisit_gap if NP > revisit_gap else NP
        s = np.where(k < first, k, k - revisit_gap + 0.5)
        side = np.where(k < first, 0.0, 0.2)
        centres = np.stack([0.30 * s, 0.05 * np.sin(0.3 * s) + side, 0.02 * s], axis=1)
        yaw = 0.01 * s
        order_key = s
    else:
        raise KeyError(pattern)
    Rcw, tcw = _poses_from(centres, yaw)
    by_path = np.argsort(order_key, kind="stable") if order_key is not None else None
    path_rank = np.argsort(by_path) if by_path is not None else None

    pts, e_pose, e_point, e_uv = [], [], [], []
    n_kept = 0
    while n_kept < n_points:
        m = max(256, (n_points - n_kept) * 2)
        anchor = rng.integers(0, NP, size=m)
        depth = rng.uniform(6.0 if pattern == "hub" else 4.0, 30.0, size=m)
        u = rng.uniform(0.0, WIDTH, size=m); v = rng.uniform(0.0, HEIGHT, size=m)
        run = rng.integers(run_lo, run_hi + 1, size=m)
        off = rng.integers(0, run_hi + 1, size=m)
        Xc = np.stack([(u - CX) / FX * depth, (v - CY) / FY * depth, depth], axis=1)
        Xw = np.einsum('mji,mj->mi', Rcw[anchor], Xc - tcw[anchor])        # Rcw^T (Xc - t)
        Y = np.einsum('kij,mj->mki', Rcw, Xw) + tcw[None, :, :]             # (m, NP, 3): the candidates in every camera
        z = Y[:, :, 2]
        zs = np.where(z > 0.1, z, 1.0)
        uu = FX * Y[:, :, 0] / zs + CX; vv = FY * Y[:, :, 1] / zs + CY
        vis = (z > 0.1) & (uu >= 0) & (uu < WIDTH) & (vv >= 0) & (vv < HEIGHT)
        for j in range(m):
            if n_kept >= n_points:
                break
            if pattern == "hub":
                cand = np.flatnonzero(vis[j])
                if len(cand) < min_obs:
                    continue
                ks = np.sort(rng.choice(cand, size=min(int(run[j]), len(cand)), replace=False))
            else:
                a = int(path_rank[anchor[j]])
                first_r = a - int(off[j]) % int(run[j])
                ranks = [r for r in range(first_r, first_r + int(run[j])) if 0 <= r < NP]
                ks = np.sort([int(by_path[r]) for r in ranks if vis[j, by_path[r]]])
            if len(ks) < min_obs:
                continue
            pts.append(Xw[j])
            for kk in ks:
                e_pose.append(int(kk)); e_point.append(n_kept); e_uv.append((uu[j, kk], vv[j, kk]))
            n_kept += 1

    truth_points = np.array(pts)
    edge_pose = np.array(e_pose, dtype=np.int32); edge_point = np.array(e_point, dtype=np.int32)
    obs = np.array(e_uv, dtype=np.float64)
    E = len(edge_pose)
    obs = obs + rng.normal(0.0, pix_sigma, size=(E, 2))
    is_out = rng.random(E) < outlier_frac
    mag = rng.uniform(5.0, 30.0, size=E); ang = rng.uniform(0.0, 2 * np.pi, size=E)
    obs[is_out] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)[is_out]

    truth_poses = np.zeros((NP, 7)); poses = np.zeros((NP, 7))
    fixed = np.zeros(NP, dtype=np.uint8); fixed[:n_fixed] = 1
    for i in range(NP):
        truth_poses[i, :4] = quat_from_R(Rcw[i]); truth_poses[i, 4:] = tcw[i]
        if fixed[i]:
            poses[i] = truth_poses[i]
        else:
            dR = _rodrigues(np.deg2rad(rot_sigma_deg) * rng.normal(size=3))
            poses[i, :4] = quat_from_R(dR @ Rcw[i]); poses[i, 4:] = tcw[i] + trans_sigma * rng.normal(size=3)
    points = truth_points + point_sigma * rng.normal(size=truth_points.shape)
    poses = _f32(poses)
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    return Window(poses=poses, pose_fixed=fixed, points=_f32(points), edge_pose=edge_pose, edge_point=edge_point,
                  obs=_f32(obs), inv_sigma2=np.ones(E), truth_poses=truth_poses, truth_points=truth_points,
                  meta=dict(seed=seed, K=n_free, F=n_fixed, P=n_points, E=E, outliers=int(is_out.sum()), pattern=pattern))


def shuffle_ids(w: Window, seed: int) -> Window:
    """The same graph with the keyframe ids permuted (fixed flags, estimates and observations follow their keyframe); edges
    re-sorted into the reference's order (point ascending, then keyframe id ascending)."""
    rng = np.random.default_rng(seed)
    NP = w.n_poses
    new_of_old = rng.permutation(NP)                    # keyframe `old` becomes id new_of_old[old]
    old_of_new = np.argsort(new_of_old)
    ep = new_of_old[w.edge_pose].astype(np.int32)
    order = np.lexsort((ep, w.edge_point))
    meta = dict(w.meta); meta["pattern"] = (meta.get("pattern", "run") + "+shuffled"); meta["id_perm"] = new_of_old
    return Window(poses=w.poses[old_of_new], pose_fixed=w.pose_fixed[old_of_new], points=w.points,
                  edge_pose=ep[order], edge_point=w.edge_point[order], obs=w.obs[order], inv_sigma2=w.inv_sigma2[order],
                  cam=w.cam, huber_delta=w.huber_delta, chi2_gate=w.chi2_gate, max_iters=w.max_iters,
                  truth_poses=None if w.truth_poses is None else w.truth_poses[old_of_new], truth_points=w.truth_points,
                  meta=meta, obs_right=None if w.obs_right is None else w.obs_right[order], bf=w.bf)


def mixed_cameras(w: Window, seed: int, models=((320.0, 320.0, 320.0, 240.0), (400.0, 410.0, 330.0, 250.0), (281.5, 279.25, 311.0, 236.5)),
                  bf_scale=(1.0, 1.25, 0.8)) -> Window:
    """The same window seen through DIFFERENT cameras: every keyframe draws one of `models` (and a baseline factor), its
    observations are mapped pixel by pixel - u' = fx' (u - cx) / fx + cx', u_r' = u' - (bf' / bf) (u - u_r) - so geometry,
    noise and outliers carry over.  The reference gives every edge its keyframe's camera (src/Optimizer.cc:664, 690-695);
    `cam` / `bf` of the result are deliberately useless (the first model / 0) so that a path reading them shows up."""
    import dataclasses
    rng = np.random.default_rng(seed)
    NP = w.n_poses
    pick = rng.integers(0, len(models), NP)
    pick[: len(models)] = np.arange(len(models))[: min(len(models), NP)]            # every model occurs
    cam_kf = _f32(np.asarray(models)[pick])
    fx, fy, cx, cy = w.cam
    k = cam_kf[w.edge_pose]
    obs = np.stack([k[:, 0] * (w.obs[:, 0] - cx) / fx + k[:, 2], k[:, 1] * (w.obs[:, 1] - cy) / fy + k[:, 3]], axis=1)
    out = dataclasses.replace(w, obs=_f32(obs), cam=tuple(float(v) for v in cam_kf[0]), cam_kf=cam_kf)
    if w.obs_right is not None:
        bf_kf = _f32(w.bf * np.asarray(bf_scale)[pick])
        st = w.obs_right >= 0
        ur = np.where(st, obs[:, 0] - (bf_kf[w.edge_pose] / w.bf) * (w.obs[:, 0] - w.obs_right), -1.0)
        # (a disparity that leaves the image on the left is no stereo observation any more)
        ur = np.where(st & (ur >= 0), ur, -1.0)
        out = dataclasses.replace(out, obs_right=np.where(ur >= 0, _f32(ur), -1.0), bf=0.0, bf_kf=bf_kf)
    return out


# ---------------------------------------------------------------------------------------------
# Pyramid levels.  Every edge of the reference's local BA carries inv_sigma2 = mvInvLevelSigma2[octave] of its keypoint
# (src/Optimizer.cc:657-658, 685-687, 724-725); the generators above give every edge the weight 1.
# ---------------------------------------------------------------------------------------------
def level_scale_factors(n_levels: int = 8, scale: float = 1.2, dtype=np.float32) -> np.ndarray:
    """mvScaleFactors as the reference's extractor builds them: s[0] = 1, s[i] = s[i-1] * scale, every product rounded to
    `dtype` (the extractor works in float; float64 gives the table in double)."""
    s = np.ones(n_levels, dtype=dtype)
    for i in range(1, n_levels):
        s[i] = s[i - 1] * dtype(scale)
    return s


def level_inv_sigma2(n_levels: int = 8, scale: float = 1.2) -> np.ndarray:
    """mvInvLevelSigma2 widened to double: inv[i] = 1.0f / (s[i] * s[i]) in float, then the cast the edge's
    `const float &invSigma2` goes through (src/Optimizer.cc:657)."""
    s = level_scale_factors(n_levels, scale, np.float32)
    return (np.float32(1.0) / (s * s)).astype(np.float64)


def with_levels(w: Window, seed: int, n_levels: int = 8, scale: float = 1.2):
    """A copy of `w` whose edges sit on pyramid levels drawn independently with p(l) ~ 0.75^l (most keypoints come from the
    fine levels, all levels occur), inv_sigma2 taken per edge from level_inv_sigma2().  -> (window, levels (E,) int32)."""
    import copy
    rng = np.random.default_rng(seed)
    p = 0.75 ** np.arange(n_levels)
    levels = rng.choice(n_levels, size=w.n_edges, p=p / p.sum()).astype(np.int32)
    out = copy.deepcopy(w)
    out.inv_sigma2 = level_inv_sigma2(n_levels, scale)[levels]
    out.meta = dict(out.meta, level_seed=seed, n_levels=n_levels)
    return out, levels


# ---------------------------------------------------------------------------------------------
# A change of world frame.  Every generator in this file builds its cameras as small rotations about the identity (a yaw
# about y, a few hundredths of a radian per axis): quaternions with w ~ 1, rotation matrices with positive trace.  For a rigid
# motion G = (Rg, tg) the points become X' = Rg X + tg and the poses Tcw' = Tcw o G^-1 (R' = R Rg^T, t' = t - R' tg); the
# observations stay.  It is the same optimisation problem, posed with cameras in general position.  The transform is made
# in double and nothing is rounded to float32 again, so a solver's result maps back to the un-gauged one to rounding.
# G^-1 = (Rg^T, -Rg^T tg) maps back.
# ---------------------------------------------------------------------------------------------
def gauge_rotation(axis, angle_deg: float):
    """Rotation by angle_deg about `axis` (any length)."""
    a = np.asarray(axis, np.float64)
    return _rodrigues(np.deg2rad(angle_deg) * a / np.linalg.norm(a))


def regauge_points(X, Rg, tg=(0.0, 0.0, 0.0)):
    return np.asarray(X, np.float64) @ np.asarray(Rg).T + np.asarray(tg, np.float64)


def regauge_poses(poses, Rg, tg=(0.0, 0.0, 0.0), flip_every: int = 0, renormalise: bool = True):
    """(N, 7) poses Tcw in the new world frame.  The quaternions come back unit with w >= 0, except: flip_every = n negates
    the quaternion of every n-th pose (1, 1 + n, ...: the same rotation, w < 0); renormalise=False scales every quaternion by
    the norm its float32 rounding has (off unit by ~3e-8: what a caller that widens a float quaternion hands over; the
    direction stays the exact one)."""
    poses = np.asarray(poses, np.float64)
    tg = np.asarray(tg, np.float64)
    out = np.zeros_like(poses)
    for i, p in enumerate(poses):
        R2 = R_from_quat(p[:4] / np.linalg.norm(p[:4])) @ np.asarray(Rg).T
        q = quat_from_R(R2)
        out[i, 4:] = p[4:] - R_from_quat(q) @ tg
        if flip_every and i % flip_every == flip_every - 1:
            q = -q
        if not renormalise:
            q = q * np.linalg.norm(_f32(q))
        out[i, :4] = q
    return out


def regauge(w: Window, Rg, tg=(0.0, 0.0, 0.0), flip_every: int = 0, renormalise: bool = True) -> Window:
    """The window `w` in the world frame moved by G = (Rg, tg): estimates and truth follow, everything else is shared."""
    import dataclasses
    meta = dict(w.meta); meta["regauged"] = True
    return dataclasses.replace(
        w, poses=regauge_poses(w.poses, Rg, tg, flip_every, renormalise), points=regauge_points(w.points, Rg, tg),
        truth_poses=None if w.truth_poses is None else regauge_poses(w.truth_poses, Rg, tg),
        truth_points=None if w.truth_points is None else regauge_points(w.truth_points, Rg, tg), meta=meta)


def regauge_frame(f: dict, Rg, tg=(0.0, 0.0, 0.0), flip: bool = False, renormalise: bool = True) -> dict:
    """A make_frame() operand in the moved world frame: Xw, pose0 and truth follow."""
    out = dict(f)
    out["Xw"] = regauge_points(f["Xw"], Rg, tg)
    out["pose0"] = regauge_poses(f["pose0"][None], Rg, tg, 1 if flip else 0, renormalise)[0]
    out["truth"] = regauge_poses(f["truth"][None], Rg, tg)[0]
    return out


def regauge_triangulation(sc: dict, Rg, tg=(0.0, 0.0, 0.0), flip_every: int = 0) -> dict:
    """A make_triangulation() scene in the moved world frame: the views' poses and the truth follow.  (The DLT minimises
    over unit homogeneous 4-vectors: a rotation of the world is orthogonal on them and leaves its result alone, a translation
    is not and changes what ill-posed matches give - in the reference too.)"""
    out = dict(sc)
    out["views"] = dict(sc["views"], poses=regauge_poses(sc["views"]["poses"], Rg, tg, flip_every))
    out["truth"] = regauge_points(sc["truth"], Rg, tg)
    return out


# ---------------------------------------------------------------------------------------------
# A change of map scale and of world origin.  Every generator in this file puts its cameras within a few metres of the origin,
# its points 4 - 30 units deep and its baselines at 0.3 units.  A monocular map is rescaled to median depth 1 when it is made
# (movba_init_map), and a trajectory runs hundreds of units away from where it started.  For X' = s X + c the poses keep R and
# get t' = s t - R c; every length scales with s, a stereo baseline (bf, bf_kf) among them; observations, weights and cameras
# stay.  It is the same optimisation problem in other units - but not the same LM path when s != 1: the damping lambda I is
# not scale-covariant.  Made in double, nothing rounded to float32 again (as regauge).  unsimilarity_* map results back.
# ---------------------------------------------------------------------------------------------
def similarity_points(X, s: float, c=(0.0, 0.0, 0.0)):
    return s * np.asarray(X, np.float64) + np.asarray(c, np.float64)


def similarity_poses(poses, s: float, c=(0.0, 0.0, 0.0)):
    """(N, 7) poses Tcw in the world X' = s X + c: the quaternions as they are, t' = s t - R c."""
    out = np.array(poses, np.float64)
    c = np.asarray(c, np.float64)
    for i, p in enumerate(out):
        out[i, 4:] = s * p[4:] - R_from_quat(p[:4] / np.linalg.norm(p[:4])) @ c
    return out


def unsimilarity_points(X, s: float, c=(0.0, 0.0, 0.0)):
    """a result of the transformed problem in the generator's world: X = (X' - c) / s"""
    return (np.asarray(X, np.float64) - np.asarray(c, np.float64)) / s


def unsimilarity_poses(poses, s: float, c=(0.0, 0.0, 0.0)):
    """... t = (t' + R c) / s"""
    out = np.array(poses, np.float64)
    c = np.asarray(c, np.float64)
    for i, p in enumerate(out):
        out[i, 4:] = (p[4:] + R_from_quat(p[:4] / np.linalg.norm(p[:4])) @ c) / s
    return out


def similarity(w: Window, s: float, c=(0.0, 0.0, 0.0)) -> Window:
    """The window `w` in the world X' = s X + c: estimates, truth and stereo baselines follow, everything else is shared."""
    import dataclasses
    meta = dict(w.meta); meta["similarity"] = (float(s), tuple(float(v) for v in c))
    return dataclasses.replace(
        w, poses=similarity_poses(w.poses, s, c), points=similarity_points(w.points, s, c),
        truth_poses=None if w.truth_poses is None else similarity_poses(w.truth_poses, s, c),
        truth_points=None if w.truth_points is None else similarity_points(w.truth_points, s, c),
        bf=s * w.bf, bf_kf=None if w.bf_kf is None else s * np.asarray(w.bf_kf, np.float64), meta=meta)


def similarity_frame(f: dict, s: float, c=(0.0, 0.0, 0.0)) -> dict:
    """A make_frame() operand in the world X' = s X + c: Xw, pose0 and truth follow."""
    out = dict(f)
    out["Xw"] = similarity_points(f["Xw"], s, c)
    out["pose0"] = similarity_poses(f["pose0"][None], s, c)[0]
    out["truth"] = similarity_poses(f["truth"][None], s, c)[0]
    return out


def pattern_cfg(name: str, seed: int | None = None) -> Window:
    """cfg3-sized windows (50 + 10 keyframes x 20 000 map points) of the other covisibility patterns."""
    if name == "hub":
        return make_pattern_window("hub", 50, 10, 20000, 3001 if seed is None else seed)
    if name == "revisit":
        return make_pattern_window("revisit", 50, 10, 20000, 3002 if seed is None else seed, run_lo=2, run_hi=10)
    if name == "shuffled":
        return shuffle_ids(cfg("cfg3"), 3003 if seed is None else seed)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------
# Keyframe pairs with matches to triangulate: the operand of movba_triangulate, i.e. what the loop of
# LocalMapping::CreateNewMapPoints sees (/root/reference/src/LocalMapping.cc:263-476) after neighbour selection and matching.
# ---------------------------------------------------------------------------------------------
TRI_KINDS = ("normal", "mismatch", "behind_both", "behind_view2", "far", "depth_zero", "depth_negative", "wide_rays", "w_zero")


def make_triangulation(n_pairs: int, n_per_pair, seed: int, stereo: bool = False, stereo_frac: float = 1.0,
                       mismatch_frac: float = 0.05, special_frac: float = 0.01, pix_sigma: float = 0.5, bf: float = 120.0,
                       far_threshold: float = 40.0, noise: bool = True) -> dict:
    """A current keyframe (view 0) and n_pairs neighbours (views 1 .. n_pairs; pair p = (0, p + 1)) at baselines of 0.2 - 1.5 m,
    n_per_pair matches each (an int, or one size per pair; 0 gives an empty pair).  Map points are drawn in the current
    keyframe's image at depths of 4 - 30 m and projected into the neighbour; 0.5 px noise on both observations; everything is
    rounded to float32 and widened, as the reference's floats arrive at the boundary.  A share of the matches are gross
    mismatches (the second observation anywhere in the image), and `special_frac` of them each are placed so that every
    reachable reject occurs: behind both cameras, between the two cameras of a neighbour that lies ahead (behind view 2),
    beyond far_threshold, and with stereo=True a stereo depth of zero / below zero and rays more than 90 degrees apart (a
    stereo observation whose parallax test fails).  The first neighbour is a pure sideways translation of the (identity)
    current keyframe; its first match observes the principal point in both: the DLT's null vector has w = 0 exactly.
    stereo: `stereo_frac` of the observations of either view that are closer than 12 m carry mvuRight / mvDepth (u_r = u - bf / z + noise, depth =
    bf / (u - u_r)), the others -1.  -> dict(views, pairs, matches, reproj_gate, far_threshold, truth (M, 3), kind (M,):
    index into TRI_KINDS): views / pairs / matches are the arguments of capi.Solver.triangulate."""
    rng = np.random.default_rng(seed)
    sizes = np.full(n_pairs, n_per_pair, dtype=np.int64) if np.isscalar(n_per_pair) else np.asarray(n_per_pair, dtype=np.int64)
    assert len(sizes) == n_pairs
    NV = n_pairs + 1
    # views: the current keyframe at the origin with identity rotation; neighbours to the side / ahead, small yaw
    k = np.arange(NV, dtype=np.float64)
    base = rng.uniform(0.2, 1.5, NV) * np.where(rng.random(NV) < 0.5, -1.0, 1.0)
    ahead = np.where(k % 4 == 2, rng.uniform(0.8, 1.2, NV), rng.uniform(-0.1, 0.1, NV))       # every fourth neighbour lies ahead
    centres = np.stack([base, rng.uniform(-0.1, 0.1, NV), ahead], axis=1)
    yaw = rng.uniform(-0.05, 0.05, NV)
    centres[0] = 0.0; yaw[0] = 0.0
    if NV > 1:
        centres[1] = (0.5, 0.0, 0.0); yaw[1] = 0.0
    Rcw, tcw = _poses_from(centres, yaw)
    poses = np.zeros((NV, 7))
    for i in range(NV):
        poses[i, :4] = quat_from_R(Rcw[i]); poses[i, 4:] = tcw[i]
    poses = _f32(poses)
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    Rcw = np.stack([R_from_quat(q) for q in poses[:, :4]]); tcw = poses[:, 4:].copy()      # (the geometry the observations see)
    cam = np.tile(np.array([FX, FY, CX, CY]), (NV, 1))
    b = bf / FX

    pair_view = np.stack([np.zeros(n_pairs, np.int32), np.arange(1, NV, dtype=np.int32)], axis=1) if n_pairs else np.zeros((0, 2), np.int32)
    pair_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M = int(pair_ptr[-1])
    v2 = np.repeat(pair_view[:, 1], sizes) if M else np.zeros(0, np.int32)
    first_of_pair = np.zeros(M, bool)
    first_of_pair[pair_ptr[:-1][sizes > 0]] = True

    # kinds
    kind = np.zeros(M, np.int64)
    r = rng.random(M)
    edges = mismatch_frac + special_frac * np.arange(0, 8)
    kind[r < edges[0]] = 1
    for j, name in enumerate(("behind_both", "behind_view2", "far") + (("depth_zero", "depth_negative", "wide_rays") if stereo else ())):
        kind[(r >= edges[j]) & (r < edges[j + 1])] = TRI_KINDS.index(name)
    ahead_of = centres[v2, 2] > 0.5 if M else np.zeros(0, bool)
    kind[(kind == TRI_KINDS.index("behind_view2")) & ~ahead_of] = 0
    if M and NV > 1 and sizes[0] > 0:
        kind[0] = TRI_KINDS.index("w_zero")

    u = rng.uniform(0.0, WIDTH, M); v = rng.uniform(0.0, HEIGHT, M)
    depth = rng.uniform(4.0, 30.0, M)
    depth = np.where(kind == TRI_KINDS.index("far"), rng.uniform(60.0, 100.0, M), depth)
    depth = np.where(kind == TRI_KINDS.index("behind_both"), -depth, depth)
    depth = np.where(kind == TRI_KINDS.index("behind_view2"), rng.uniform(0.3, 0.6, M), depth)
    Xc1 = np.stack([(u - CX) / FX * depth, (v - CY) / FY * depth, depth], axis=1)
    Xw = np.einsum('ji,mj->mi', Rcw[0], Xc1 - tcw[0])
    Xc2 = np.einsum('mij,mj->mi', Rcw[v2], Xw) + tcw[v2]
    z2 = Xc2[:, 2]
    z2s = np.where(np.abs(z2) > 1e-9, z2, 1e-9)
    obs1 = np.stack([u, v], axis=1)
    obs2 = np.stack([FX * Xc2[:, 0] / z2s + CX, FY * Xc2[:, 1] / z2s + CY], axis=1)
    if noise:
        obs1 = obs1 + rng.normal(0.0, pix_sigma, (M, 2)); obs2 = obs2 + rng.normal(0.0, pix_sigma, (M, 2))
    mm = kind == 1
    obs2[mm] = np.stack([rng.uniform(0.0, WIDTH, M), rng.uniform(0.0, HEIGHT, M)], axis=1)[mm]
    wide = kind == TRI_KINDS.index("wide_rays")
    obs1[wide, 0] = rng.uniform(-40.0, -10.0, M)[wide]; obs2[wide, 0] = rng.uniform(WIDTH + 10.0, WIDTH + 40.0, M)[wide]
    wz = kind == TRI_KINDS.index("w_zero")
    obs1[wz] = (CX, CY); obs2[wz] = (CX, CY)

    matches = dict(obs1=_f32(obs1), obs2=_f32(obs2))
    views = dict(poses=poses, cam=cam)
    if stereo:
        def right(obs_u, z, is_view1):
            zs = np.where(z > 0.1, z, 1.0)
            ur = obs_u - bf / zs + (rng.normal(0.0, pix_sigma, M) if noise else 0.0)
            st = (rng.random(M) < stereo_frac) & (z > 0.1) & (z < 12.0) & (ur >= 0.0) & ~wz     # (close points only, as ThDepth has it)
            if not is_view1:
                st &= ~wide                 # (rays wide apart, stereo in view 1 only: neither parallax test holds)
            else:
                st |= wide | (kind == TRI_KINDS.index("depth_zero")) | (kind == TRI_KINDS.index("depth_negative"))
            ur = _f32(np.where(st, np.maximum(ur, 0.0), -1.0))
            d = np.where(st, bf / np.maximum(obs_u - ur, 1e-3), -1.0)
            return ur, d
        ur1, d1 = right(matches["obs1"][:, 0], Xc1[:, 2], True)
        ur2, d2 = right(matches["obs2"][:, 0], z2, False)
        d1 = np.where(kind == TRI_KINDS.index("depth_zero"), 0.0, d1)
        d1 = np.where(kind == TRI_KINDS.index("depth_negative"), -1.0, d1)
        matches.update(ur1=ur1, ur2=ur2, depth1=_f32(d1), depth2=_f32(d2))
        views.update(bf=_f32(np.full(NV, bf)), b=_f32(np.full(NV, b)))
    return dict(views=views, pairs=dict(pair_view=pair_view, pair_ptr=pair_ptr), matches=matches, reproj_gate=5.0,
                far_threshold=far_threshold, truth=Xw, kind=kind, meta=dict(seed=seed, n_pairs=n_pairs, M=M, stereo=stereo))


def concat_triangulations(scenes) -> dict:
    """Several make_triangulation scenes as ONE call's arguments (view indices shifted, pair_ptr continued): the keyframes of
    several sessions at once.  Scenes without stereo arrays get monocular ones (-1) when any other has them."""
    any_st = any("ur1" in s["matches"] for s in scenes)
    poses, cam, bfs, bs, pv, sizes, truth, kind = [], [], [], [], [], [], [], []
    m = {k: [] for k in ("obs1", "obs2", "ur1", "ur2", "depth1", "depth2")}
    off = 0
    for s in scenes:
        nv = len(s["views"]["poses"]); n = int(s["pairs"]["pair_ptr"][-1])
        poses.append(s["views"]["poses"]); cam.append(s["views"]["cam"])
        bfs.append(s["views"].get("bf", np.zeros(nv))); bs.append(s["views"].get("b", np.zeros(nv)))
        pv.append(s["pairs"]["pair_view"] + off); sizes.append(np.diff(s["pairs"]["pair_ptr"]))
        off += nv
        for k in ("obs1", "obs2"):
            m[k].append(s["matches"][k])
        for k in ("ur1", "ur2", "depth1", "depth2"):
            m[k].append(s["matches"].get(k, np.full(n, -1.0)))
        truth.append(s["truth"]); kind.append(s["kind"])
    views = dict(poses=np.concatenate(poses), cam=np.concatenate(cam))
    matches = dict(obs1=np.concatenate(m["obs1"]), obs2=np.concatenate(m["obs2"]))
    if any_st:
        views.update(bf=np.concatenate(bfs), b=np.concatenate(bs))
        matches.update({k: np.concatenate(m[k]) for k in ("ur1", "ur2", "depth1", "depth2")})
    pair_ptr = np.concatenate([[0], np.cumsum(np.concatenate(sizes))]).astype(np.int32)
    return dict(views=views, pairs=dict(pair_view=np.concatenate(pv).astype(np.int32), pair_ptr=pair_ptr), matches=matches,
                reproj_gate=scenes[0]["reproj_gate"], far_threshold=scenes[0]["far_threshold"], truth=np.concatenate(truth),
                kind=np.concatenate(kind), meta=dict(M=int(pair_ptr[-1]), n_pairs=len(pair_ptr) - 1))


TWO_VIEW_SCENES = ("general", "planar", "rotation", "forward")


def make_two_view(n_matches: int, inlier_frac: float = 0.7, noise_px: float = 0.5, seed: int = 0, scene: str = "general",
                  cam=(458.0, 457.0, 367.0, 248.0), width: int = 752, height: int = 480, roll_deg: float = 0.0) -> dict:
    """One frame pair for movba_two_view: camera 1 at the origin, camera 2 at T21 = (R, t) with |t| = 1 (the unit the call
    returns), points seen by both, noise_px of Gaussian noise on both observations; 1 - inlier_frac of the matches are gross
    mismatches (the second observation anywhere in the image).  Scenes: `general` - depths of 4 - 40 baselines, sideways
    motion with a few degrees of rotation; `planar` - every point on one slanted plane (the case an eight-point solver cannot
    do); `rotation` - zero baseline (no parallax: initialisation must fail); `forward` - motion along the optical axis.
    roll_deg: camera 2 turned by this angle about its own optical axis on top of the scene's motion (R <- Rz R, t <- Rz t,
    before projection; the returned truth includes it): 180 degrees gives a T21 whose rotation has trace ~ -1.
    -> dict(obs1, obs2 (M, 2), cam, R (3, 3), t (3,): the true T21 (t = 0 for `rotation`), X (M, 3): the points in camera 1,
    is_inlier (M,))."""
    assert scene in TWO_VIEW_SCENES
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = cam
    M = int(n_matches)
    u = rng.uniform(20, width - 20, M); v = rng.uniform(20, height - 20, M)
    if scene == "planar":
        nrm = np.array([0.3, -0.2, -1.0]); nrm /= np.linalg.norm(nrm)
        rays = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones(M)], 1)
        z = (nrm @ np.array([0.0, 0.0, 8.0])) / (rays @ nrm)            # the plane through (0, 0, 8)
    else:
        z = rng.uniform(4.0, 40.0, M)
    X = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    w = rng.uniform(-0.06, 0.06, 3)
    if scene == "rotation":
        w = rng.uniform(-0.1, 0.1, 3)
    th = np.linalg.norm(w); k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    if scene == "forward":
        t = np.array([0.05, -0.03, -1.0])
    else:
        t = np.array([-1.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
    t = t / np.linalg.norm(t)
    if scene == "rotation":
        t = np.zeros(3)
    if roll_deg != 0.0:
        Rz = _rodrigues(np.array([0.0, 0.0, np.deg2rad(roll_deg)]))
        R = Rz @ R; t = Rz @ t
    Y = X @ R.T + t
    obs1 = np.stack([u, v], 1) + rng.normal(0, noise_px, (M, 2)) if noise_px > 0 else np.stack([u, v], 1)
    obs2 = np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1)
    if noise_px > 0:
        obs2 = obs2 + rng.normal(0, noise_px, (M, 2))
    is_inlier = rng.random(M) < inlier_frac
    bad = ~is_inlier
    obs2[bad] = np.stack([rng.uniform(0, width, bad.sum()), rng.uniform(0, height, bad.sum())], 1)
    return dict(obs1=obs1, obs2=obs2, cam=tuple(float(c) for c in cam), R=R, t=t, X=X, is_inlier=is_inlier)
