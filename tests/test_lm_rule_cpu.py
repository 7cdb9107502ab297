"""The Levenberg step rule of mov-slam_amd/csrc/lm_rule.h without a GPU.

tests/lm_rule/lm_rule_main.cpp includes the header over the stand-in runtime header of tests/hipstub; it is built with the host
compiler under the sanitizers and run as a child process: the hand cases (a failed solve with a finite and with an infinite
current cost, rho == 0, a lambda that stops being finite, the last allowed trial, nu over rejections and acceptances), and
a replay of the trials the golden fixtures recorded.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

FLAGS = ["-std=c++17", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "hipstub"),
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mov-slam_amd", "csrc"), "-Wall", "-Wno-unused-function",
         "-Wno-unknown-pragmas", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0 abort_on_error=0 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1")

# lambda behind an ACCEPTED trial, relative: the fixtures cube 2 rho - 1 with a power function, lm_rule.h with t * t * t; both are
# within 2 ulp (4.5e-16) of a value of magnitude at most 1, which is subtracted from 1 to give a factor of at least 1/3: the
# two factors differ by less than 4 * 2.3e-16 / (1/3) < 3e-15 relative, and the product with lambda adds a rounding on either
# side.  1e-12 leaves that three orders of room; the run prints the worst it measures, and above 1e-13 something other than the
# cube differs.
LAMBDA_RTOL = 1e-12
FIXTURES = ("lba_hard", "lba_cameras", "lba_stereo")


@pytest.fixture(scope="module")
def lm_rule_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lm_rule") / "lm_rule_main")
    subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [os.path.join(ROOT, "tests", "lm_rule", "lm_rule_main.cpp"), "-o", exe])
    return exe


def run(exe, arg):
    r = subprocess.run([exe, arg], env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=120)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[:4000]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def test_hand_cases(lm_rule_main):
    assert run(lm_rule_main, "hand").strip() == "hand ok"


def test_replay_of_the_golden_traces(lm_rule_main, tmp_path):
    """Every trial k of the fixtures: from lam[k], rho[k], F1[k] and the carried nu the header must take the fixture's accept
    flag, after a rejection lam[k] * nu exactly (powers of two), after an acceptance the fixture's next lambda to LAMBDA_RTOL.
    The lambda behind the last trial is the fixture's final one."""
    n_rejected = n_unclamped = 0
    worst = 0.0
    for name in FIXTURES:
        _, out = load_golden(name)
        lam, rho, f1, acc = out["tr_lam"], out["tr_rho"], out["tr_f1"], out["tr_accept"]
        n = len(lam)
        assert n > 0 and len(rho) == n and len(f1) == n and len(acc) == n
        nxt = np.append(lam[1:], float(out["lam"]))
        path = str(tmp_path / (name + ".txt"))
        with open(path, "w") as fh:
            for k in range(n):
                fh.write(f"{float(lam[k])!r} {float(rho[k])!r} {float(f1[k])!r}\n")
        rows = [ln.split() for ln in run(lm_rule_main, path).strip().splitlines()]
        assert len(rows) == n and all(r[0] == "trial" for r in rows)
        nu = 2.0
        for k, (_, a, lam_next, nu_next) in enumerate(rows):
            a, lam_next, nu_next = int(a), float(lam_next), float(nu_next)
            assert a == int(acc[k]), (name, k)
            if a:
                rel = abs(lam_next - nxt[k]) / nxt[k]
                worst = max(worst, rel)
                assert rel <= LAMBDA_RTOL, (name, k, lam_next, nxt[k])
                assert nu_next == 2.0
                n_unclamped += 1.0 / 3.0 < 1.0 - (2.0 * float(rho[k]) - 1.0) ** 3 < 2.0 / 3.0
            else:
                assert lam_next == float(lam[k]) * nu and lam_next == nxt[k] and nu_next == 2.0 * nu, (name, k, lam_next, nxt[k], nu)
                n_rejected += 1
            nu = nu_next
    print(f"replay: {n_rejected} rejected trials, {n_unclamped} accepted with the factor strictly inside (1/3, 2/3); "
          f"worst relative difference of lambda behind an accepted trial {worst:.3g} (LAMBDA_RTOL {LAMBDA_RTOL:.3g})")
    assert n_rejected >= 5 and n_unclamped >= 4
