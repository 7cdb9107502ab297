"""The measurements behind the order-noise bounds of tests/test_gpu_parity.py: for each of the 14 sweep windows the oracle's own
spread over 16 within-point edge orders (tests/order_noise.py) and, with a GPU, how far each of the three solver choices is from
the oracle in every bounded quantity, as a fraction of the bound its test holds it to.
    python tests/dev/order_noise_report.py --spreads profiles/order_noise_spreads.json            (any machine)
    python tests/dev/order_noise_report.py --gpu profiles/order_noise_gpu_fractions.json          (on the GPU)
The same two records for the windows of tests/test_gpu_map_scale.py (three windows under five changes of map scale and world
origin, the four reduced solvers of test_gpu_general_position.SOLVERS), the bounds with length_unit = s:
    python tests/dev/order_noise_report.py --scale-spreads profiles/map_scale_spreads.json         (any machine)
    python tests/dev/order_noise_report.py --scale-gpu profiles/map_scale_gpu_fractions.json       (on the GPU)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mov-slam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from movba import synth
from oracle import oracle
import order_noise
import test_gpu_parity as parity

ap = argparse.ArgumentParser()
ap.add_argument("--spreads", help="write the spread records (CPU only) to this JSON file")
ap.add_argument("--gpu", help="solve on the GPU too and write the fractions of the bounds to this JSON file")
ap.add_argument("--scale-spreads", help="write the spread records of the map-scale windows (CPU only) to this JSON file")
ap.add_argument("--scale-gpu", help="solve the map-scale windows on the GPU too and write the fractions of the bounds to this JSON file")
args = ap.parse_args()
oracle.build()


def write(path, rows):
    if path:
        with open(path, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


def map_scale():
    import test_map_scale_cpu as M
    spreads, fractions = [], []
    if args.scale_gpu:
        from movba import capi
        from test_gpu_general_position import SOLVERS
        solvers = {name: capi.Solver(**kw) for name, kw in dict(SOLVERS, default={}).items()}
        solvers["banded", "kf30"] = capi.Solver(solver=2)      # (the default choice gives kf30 to the PCG: k_band forced, as the test)
    for name in M.WINDOWS:
        for t in [None] + M.T_IDS + [M.TOO_FAR]:
            s, c = (1.0, M.ZERO) if t is None else M.TRANSFORMS[t] if isinstance(t, str) else t
            label = "none" if t is None else t if isinstance(t, str) else "1e5"
            if label == "1e5" and name != "kf30":
                continue
            w, o, sp, tol = M.window(name, t), M.oracle_solve(oracle, name, t), M.spread_of(oracle, name, t), M.bounds(oracle, name, t)
            rec = dict(window=name, transform=label, s=s, c=list(c), edges=w.n_edges, accept="".join(map(str, o["trace"]["accept"])),
                       n_solves=o["n_solves"], noise_floor=order_noise.noise_floor_trial(o), lambda_0=float(o["trace"]["lam"][0]), n=sp.n, rot=sp.rot,
                       trans=sp.trans, point=sp.point, trans_over_s=sp.trans / s, point_over_s=sp.point / s, lam=sp.lam, f1=sp.f1, chi2=sp.chi2,
                       same_decisions=sp.same_decisions, bounds=dict(tol, chi2_tol=list(tol["chi2_tol"])))
            spreads.append(rec)
            print("spread", json.dumps(rec), flush=True)
            if not args.scale_gpu or label == "1e5":
                continue
            for which in (["default"] if name == "small" else list(SOLVERS)):      # (`small`: on the default solver choice only, as the test)
                r = solvers.get((which, name), solvers[which]).solve(w)
                d = order_noise.distances(r, o, w)
                fr = {k: d[k] / (tol[k][0] if k == "chi2_tol" else tol[k]) for k in d}
                rec = dict(window=name, transform=label, which=which, n_band=r["n_band"], n_direct=r["n_direct"], n_pcg_giveups=r["n_pcg_giveups"],
                           pcg_iters=r["pcg_iters"], n_solves=r["n_solves"], distance=d, fraction=fr, worst=max(fr.values()))
                fractions.append(rec)
                print("gpu", json.dumps(rec), flush=True)
    if args.scale_gpu:
        for s in solvers.values(): s.close()
    write(args.scale_spreads, spreads); write(args.scale_gpu, fractions)


if args.scale_spreads or args.scale_gpu:
    map_scale()
    if not (args.spreads or args.gpu):
        sys.exit(0)

WHICH = [("default-solver", {}), ("banded", dict(solver=2)), ("dense-direct", dict(solver=1))]
spreads, fractions = [], []
if args.gpu:
    from movba import capi
    solvers = {name: capi.Solver(**kw) for name, kw in WHICH}
for test, windows in (("band_sweep", parity.BAND_SWEEP_WINDOWS), ("long_sweeps", parity.LONG_SWEEP_WINDOWS)):
    for K, F, P, lo, hi, stereo, seed in windows:
        w = synth.make_window(K, F, P, seed=seed, run_lo=lo, run_hi=max(lo, hi), stereo_frac=stereo)
        sp = order_noise.spread(oracle, w, n=16)
        # the bounds each test holds the window to: the six older windows keep their pose bounds from the first four orders
        tol = parity._band_sweep_bounds(w, oracle)[0] if test == "band_sweep" else order_noise.tolerances(w, sp)
        rec = dict(seed=seed, window=[K, F, P, lo, hi, stereo], edges=w.n_edges, test=test, n=sp.n, rot=sp.rot, trans=sp.trans, point=sp.point,
                   lam=sp.lam, f1=sp.f1, chi2=sp.chi2, same_decisions=sp.same_decisions, first4=list(sp.first4),
                   bounds=dict(tol, chi2_tol=list(tol["chi2_tol"])))
        spreads.append(rec)
        print("spread", json.dumps(rec), flush=True)
        if not args.gpu:
            continue
        o = oracle.solve(w)
        for name, _ in WHICH:
            r = solvers[name].solve(w)
            d = order_noise.distances(r, o, w)
            fr = {k: d[k] / (tol[k][0] if k == "chi2_tol" else tol[k]) for k in d}
            rec = dict(seed=seed, which=name, test=test, n_band=r["n_band"], n_direct=r["n_direct"], n_solves=r["n_solves"], distance=d, fraction=fr,
                       worst=max(fr.values()))
            fractions.append(rec)
            print("gpu", json.dumps(rec), flush=True)
if args.gpu:
    for s in solvers.values(): s.close()
for path, rows in ((args.spreads, spreads), (args.gpu, fractions)):
    if path:
        with open(path, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
