"""Time batched equilibrium sweeps on one GPU and write profiles/equil_sweep.json.

GRI-3.0 CH4/air on a phi x T x P grid: 2^20 TP states (option 1; 500-3000 K), 2^20 HP states (option 5;
reactants at 300-1500 K) and 2^16 Chapman-Jouguet states (option 10; 300-1000 K, 0.1-10 atm).  Each sweep is
timed with device events after a warm-up launch; the inputs are on the device before the clock starts.  The
numpy reference of tests/equilibrium_reference.py solves a 4,096-state sample of each sweep on one host core
(one batched call) for the cost of a CPU solver and a cross-check.  The rates are reported, not gated.

    python scripts/equil_sweep.py [--log2-n 20] [--log2-cj 16] [--repeats 3] [--out profiles/equil_sweep.json]
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

P_ATM = 1.01325e6


def grid(mech, n_phi, n_T, n_P, phi, T, P_atm):
    g = np.stack(np.meshgrid(np.linspace(*phi, n_phi), np.linspace(*T, n_T),
                             P_ATM * np.logspace(np.log10(P_atm[0]), np.log10(P_atm[1]), n_P), indexing="ij"),
                 axis=-1).reshape(-1, 3)
    X = np.zeros((g.shape[0], mech.KK))
    X[:, mech.species.index("CH4")] = g[:, 0]
    X[:, mech.species.index("O2")] = 2.0
    X[:, mech.species.index("N2")] = 2.0 * 0.79 / 0.21
    Y = X * mech.wt
    return g[:, 1].copy(), g[:, 2].copy(), Y / Y.sum(axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--log2-cj", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-ref", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equil_sweep.json"))
    a = ap.parse_args()

    import torch

    from equilibrium_reference import EquilibriumReference
    from pychemkin_amd import _native
    from pychemkin_amd.mechanism import Mechanism

    mech = Mechanism.from_files(os.path.join(ROOT, "data", "grimech30_chem.inp"),
                                os.path.join(ROOT, "data", "grimech30_thermo.dat"))
    dm = _native.DeviceMechanism(mech.to_tables(), device=0)
    ref = EquilibriumReference(mech)

    sweeps = {
        "TP": (1, a.log2_n, dict(phi=(0.4, 3.0), T=(500.0, 3000.0), P_atm=(0.1, 100.0))),
        "HP": (5, a.log2_n, dict(phi=(0.4, 3.0), T=(300.0, 1500.0), P_atm=(0.1, 100.0))),
        "CJ": (10, a.log2_cj, dict(phi=(0.6, 2.0), T=(300.0, 1000.0), P_atm=(0.1, 10.0))),
    }
    out = {"what": "batched equilibrium sweeps, GRI-3.0 CH4/air, phi x T x P grid, one GPU, cold start",
           "device": torch.cuda.get_device_name(0), "tol": 1e-12, "max_iter": 200, "sweeps": {}}
    for name, (opt, log2n, rng) in sweeps.items():
        k = (log2n + 1) // 3
        n_phi, n_T, n_P = 1 << (log2n - 2 * k), 1 << k, 1 << k
        T, P, Y = grid(mech, n_phi, n_T, n_P, **rng)
        n = T.size
        Td, Pd, Yd = dm._dev(T), dm._dev(P), dm._dev(Y)
        od = torch.full((n,), opt, dtype=torch.int32, device=dm.device)
        dm.equil_run(od, Td, Pd, Yd)  # warm-up: module load, the mechanism's table, the allocator
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = dm.equil_run(od, Td, Pd, Yd)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        st = r["stats"].cpu().numpy()
        Tg = r["T"].cpu().numpy()
        Dg = r["detspeed"].cpu().numpy()
        idx = np.arange(0, n, max(1, n // a.n_ref))[:a.n_ref]
        t0 = time.perf_counter()
        rr = ref.solve(np.full(idx.size, opt), T[idx], P[idx], Y[idx])
        t_ref = time.perf_counter() - t0
        both = (rr["status"] == 0) & (st[idx, 1] == 0)
        s = {
            "option": opt, "states": n, "grid": {"phi": [*rng["phi"], n_phi], "T_K": [*rng["T"], n_T],
                                                 "P_atm": [*rng["P_atm"], n_P]},
            "milliseconds": ms, "milliseconds_median": float(np.median(ms)),
            "states_per_second": float(n / np.median(ms) * 1e3),
            "iterations_mean": float(st[:, 0].mean()), "iterations_max": int(st[:, 0].max()),
            "not_converged": int((st[:, 1] != 0).sum()),
            "numpy_reference": {"states": int(idx.size), "seconds": t_ref, "states_per_second": float(idx.size / t_ref),
                                "not_converged": int((rr["status"] != 0).sum()),
                                "iterations_max": int(rr["iterations"].max()),
                                "max_rel_T_difference": float(np.max(np.abs(Tg[idx][both] / rr["T"][both] - 1)))},
        }
        if opt == 10:
            s["hugoniot_points_mean"] = float(st[:, 2].mean())
            s["hugoniot_points_max"] = int(st[:, 2].max())
            s["numpy_reference"]["max_rel_D_difference"] = float(np.max(np.abs(Dg[idx][both] / rr["detspeed"][both] - 1)))
        out["sweeps"][name] = s
        print(name, json.dumps(s), flush=True)
        del Td, Pd, Yd, od, r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
