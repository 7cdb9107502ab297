"""The measurements behind the order-noise bounds of tests/test_gpu_parity.py: for each of the 14 sweep windows the oracle's own
spread over 16 within-point edge orders (tests/order_noise.py) and, with a GPU, how far each of the three solver choices is from
the oracle in every bounded quantity, as a fraction of the bound its test holds it to.
    python tests/dev/order_noise_report.py --spreads profiles/order_noise_spreads.json            (any machine)
    python tests/dev/order_noise_report.py --gpu profiles/order_noise_gpu_fractions.json          (on the GPU)"""
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
args = ap.parse_args()
oracle.build()

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
