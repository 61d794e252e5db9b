"""Time a 16,384-reactor steady-state PSR sweep on one GPU and write profiles/psr_sweep.json.

GRI-3.0 CH4/air, 300 K inlet: phi 0.6-1.4 (16 values) x tau 0.1-10 ms (32, logarithmic) x P 1-10 atm
(32, logarithmic), burnt estimate, steady-state rule 1e-8 / 1e-14, integrator 1e-8 / 1e-14.  The numpy
reference of tests/psr_reference.py solves 64 of the reactors (every 256th) on the CPU, one at a time, for
the per-reactor cost of a serial solver and a cross-check of the answers.  The rate is reported, not gated.

    python scripts/psr_sweep.py [--n-phi 16 --n-tau 32 --n-p 32] [--repeats 3] [--out profiles/psr_sweep.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-phi", type=int, default=16)
    ap.add_argument("--n-tau", type=int, default=32)
    ap.add_argument("--n-p", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-ref", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psr_sweep.json"))
    a = ap.parse_args()

    import torch

    import pychemkin_amd as ck
    from oracle.oracle import Oracle
    from psr_reference import PSRReference

    P_ATM = 1.01325e6
    chem = ck.Chemistry(label="GRI 3.0")
    chem.chemfile = os.path.join(ROOT, "data", "grimech30_chem.inp")
    chem.thermfile = os.path.join(ROOT, "data", "grimech30_thermo.dat")
    chem.preprocess()
    mech = chem.mechanism
    phi = np.linspace(0.6, 1.4, a.n_phi)
    tau = np.logspace(-4, -2, a.n_tau)
    P = P_ATM * np.logspace(0, 1, a.n_p)
    g = np.stack(np.meshgrid(phi, tau, P, indexing="ij"), axis=-1).reshape(-1, 3)
    n = g.shape[0]
    X = np.zeros((n, mech.KK))
    X[:, mech.species.index("CH4")] = g[:, 0]
    X[:, mech.species.index("O2")] = 2.0
    X[:, mech.species.index("N2")] = 2.0 * 0.79 / 0.21
    Y = X * mech.wt
    Yin = Y / Y.sum(axis=1, keepdims=True)
    batch = ck.BatchPSR(chem, devices=[0])
    t0 = time.perf_counter()
    Tg, Yg = batch.burnt_estimate(g[:, 2], Yin)
    torch.cuda.synchronize()
    t_est = time.perf_counter() - t0
    print(f"burnt estimate of {n} reactors: {t_est:.3f} s", flush=True)
    times = []
    for _ in range(a.repeats + 1):  # the first run warms up (module load, allocator)
        t0 = time.perf_counter()
        res = batch.run(300.0, g[:, 2], 1.0, tau=g[:, 1], Yin=Yin, estimate="given", T_estimate=Tg, Y_estimate=Yg)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        print(f"sweep of {n} reactors: {times[-1]:.3f} s, status counts "
              f"{ {int(v): int((res.status == v).sum()) for v in np.unique(res.status)} }, "
              f"steps mean {res.stats[:, 0].mean():.0f} max {res.stats[:, 0].max()}", flush=True)
    times = times[1:]
    status = {int(s): int((res.status == s).sum()) for s in np.unique(res.status)}
    # the serial numpy reference on a subset
    orc = Oracle(mech)
    idx = np.arange(0, n, max(1, n // a.n_ref))[:a.n_ref]
    t0 = time.perf_counter()
    dT, nfail = [], 0
    for i in idx:
        try:
            y, _ = PSRReference(orc, g[i, 2], 300.0, Yin[i], 1.0, tau=g[i, 1]).solve(Tg[i], Yg[i])
            dT.append(abs(y[0] / res.T[i] - 1.0))
        except RuntimeError:
            nfail += 1
    t_ref = time.perf_counter() - t0
    out = {
        "what": "steady-state PSR sweep, GRI-3.0 CH4/air, 300 K inlet, burnt estimate, one GPU",
        "device": torch.cuda.get_device_name(0),
        "reactors": n, "grid": {"phi": [0.6, 1.4, a.n_phi], "tau_s": [1e-4, 1e-2, a.n_tau], "P_atm": [1.0, 10.0, a.n_p]},
        "ss_rtol": batch.ss_rtol, "ss_atol": batch.ss_atol, "rtol": batch.cfg.rtol, "atol": batch.cfg.atol,
        "seconds": times, "seconds_median": float(np.median(times)),
        "reactors_per_second": float(n / np.median(times)),
        "burnt_estimate_seconds": t_est,
        "status_counts": status, "ignited": int((res.T > 1000.0).sum()),
        "steps_mean": float(res.stats[:, 0].mean()), "steps_max": int(res.stats[:, 0].max()),
        "rhs_mean": float(res.stats[:, 1].mean()), "resid_max_steady": float(res.resid[res.status == 0].max()),
        "numpy_reference": {"reactors": int(len(idx)), "seconds": t_ref, "reactors_per_second": float(len(idx) / t_ref),
                            "not_converged": nfail, "max_rel_T_difference": float(max(dT)) if dT else None},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
