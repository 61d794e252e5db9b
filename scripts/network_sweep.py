"""Time 4,096 three-reactor combustor networks (12,288 PSRs) on one GPU and write profiles/network_sweep.json.

GRI-3.0, the PSRnetwork topology (mixing zone -> flame zone -> third zone, which returns a share of its outflow
15 : 85 to the first two): phi 0.5-0.8 (16 values) x recirculated fraction of the flame zone's outflow 0.02-0.3
(16) x residence-time scale 0.8-1.5 (16), 10 atm, burnt estimate, tear tolerance 1e-6 / 1e-8, steady-state rule
1e-8 / 1e-14.  Reported, not gated:

  * networks/s of BatchPSRNetwork.run (one warm-up, then --repeats timed runs, median and spread), mean and
    maximum sweeps;
  * the share of the kernels' time in the PSR kernel and in the network's own kernels, from the kernel-stats CSV of
    a separate profiled run (--kernel-stats; without it: not measured), and the per-sweep host read-back measured
    as the wall time of a run minus the kernels' time when that CSV is given;
  * the numpy reference (tests/network_reference.py) on a 64-network subsample, one host core;
  * the ReactorNetwork drop-in looped over 16 of the networks, one at a time.

    python scripts/network_sweep.py [--n 16] [--repeats 3] [--n-ref 64] [--n-dropin 16] [--kernel-stats CSV]
"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def kernel_shares(path):
    """{"psr", "network", "other"}: total kernel nanoseconds by family from a rocprofv3 --stats kernel CSV."""
    tot = {"psr": 0.0, "network": 0.0, "other": 0.0}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
            # reactor_kernel<N, PL, F64, PSR>: only the PSR = true instantiations belong to the network's solves (the
            # burnt estimate's closed reactors run outside the timed runs)
            fam = "network" if "net_" in name else ("psr" if re.search(r"reactor_kernel<\d+, \w+, \w+, true>", name) else "other")
            tot[fam] += ns
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16, help="values per axis (n^3 networks)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-ref", type=int, default=64)
    ap.add_argument("--n-dropin", type=int, default=16)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--runs-only", action="store_true", help="the timed runs only (for a profiled run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_sweep.json"))
    a = ap.parse_args()

    import torch

    import pychemkin_amd as ck
    from conftest import P_ATM
    from network_cases import combustor, pack_ext
    from network_reference import NetworkReference
    from oracle.oracle import Oracle

    chem = ck.Chemistry(label="GRI 3.0")
    chem.chemfile = os.path.join(ROOT, "data", "grimech30_chem.inp")
    chem.thermfile = os.path.join(ROOT, "data", "grimech30_thermo.dat")
    chem.preprocess()
    mech = chem.mechanism
    grid = np.stack(np.meshgrid(np.linspace(0.5, 0.8, a.n), np.linspace(0.02, 0.3, a.n), np.linspace(0.8, 1.5, a.n),
                                indexing="ij"), axis=-1).reshape(-1, 3)
    base_tau = np.array([0.5e-3, 1.5e-3, 1.5e-3])
    cases = [combustor(mech, phi=p, to_third=0.3, back=r / 0.3, tau=base_tau * s) for p, r, s in grid]
    n = len(cases)
    packed = [pack_ext(c["ext"], mech.KK) for c in cases]
    P = np.full((n, 3), 10.0 * P_ATM)
    args = (P, np.stack([c["split"] for c in cases]), np.stack([p[0] for p in packed]), np.stack([p[1] for p in packed]))
    kw = dict(ext_Y=np.stack([p[2] for p in packed]), tau=np.stack([c["tau"] for c in cases]),
              tear=np.stack([c["tear"] for c in cases]))
    tol = dict(ss_rtol=1e-8, ss_atol=1e-14, rtol=1e-8, atol=1e-14, tear_rtol=1e-6, tear_atol=1e-8)
    batch = ck.BatchPSRNetwork(chem, 3, devices=[0], **tol)
    # the burnt estimate once, outside the timed runs: one closed-reactor launch over the distinct feeds
    t0 = time.perf_counter()
    feed = np.einsum("ns,nsk->nk", args[2].reshape(n, -1), kw["ext_Y"].reshape(n, -1, mech.KK))
    feed /= args[2].reshape(n, -1).sum(axis=1, keepdims=True)
    Tb, Yb = ck.BatchPSR(chem, devices=[0]).burnt_estimate(P[:, 0], feed)
    torch.cuda.synchronize()
    t_est = time.perf_counter() - t0
    est = dict(estimate="given", T_estimate=np.repeat(Tb[:, None], 3, axis=1), Y_estimate=np.repeat(Yb[:, None], 3, axis=1))
    times = []
    for _ in range(a.repeats + 1):   # the first run warms up (code objects, allocator)
        t0 = time.perf_counter()
        res = batch.run(*args, **kw, **est)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        print(f"{n} networks: {times[-1]:.3f} s, status { {int(v): int((res.status == v).sum()) for v in np.unique(res.status)} }, "
              f"sweeps mean {res.sweeps.mean():.2f} max {res.sweeps.max()}", flush=True)
    times = times[1:]
    if a.runs_only:
        return
    med = float(np.median(times))
    out = {
        "what": "4,096 three-reactor GRI-3.0 combustor networks (PSRnetwork topology), burnt estimate, one GPU",
        "device": torch.cuda.get_device_name(0), "networks": n, "reactors": 3 * n,
        "grid": {"phi": [0.5, 0.8, a.n], "recirculated_fraction": [0.02, 0.3, a.n], "tau_scale": [0.8, 1.5, a.n]},
        **tol, "seconds": times, "seconds_median": med, "seconds_spread": float(max(times) - min(times)),
        "networks_per_second": n / med, "burnt_estimate_seconds": t_est,
        "status_counts": {int(s): int((res.status == s).sum()) for s in np.unique(res.status)},
        "sweeps_mean": float(res.sweeps.mean()), "sweeps_max": int(res.sweeps.max()),
        "tear_residual_max": float(res.tear_resid.max()),
    }
    if a.kernel_stats:
        ks = kernel_shares(a.kernel_stats)
        runs = a.repeats + 1   # the profiled run times the same runs, warm-up included
        out["kernel_seconds_per_run"] = {k: v * 1e-9 / runs for k, v in ks.items()}
        kt = (ks["psr"] + ks["network"]) * 1e-9 / runs
        out["share_of_wall_time"] = {"psr_kernel": ks["psr"] * 1e-9 / runs / med, "network_kernels": ks["network"] * 1e-9 / runs / med,
                                     "host_copies_and_read_back": max(0.0, 1.0 - kt / med)}
    else:
        out["share_of_wall_time"] = "not measured (needs the kernel-stats CSV of a separate profiled run)"
    # the numpy reference on a subsample, one core, from the same estimates
    orc = Oracle(mech)
    idx = np.arange(0, n, max(1, n // a.n_ref))[:a.n_ref]
    t0, dT, nfail = time.perf_counter(), [], 0
    for i in idx:
        c = cases[i]
        try:
            T, _, _, _ = NetworkReference(orc, c["P"], c["split"], c["ext"], tau=c["tau"]).solve(
                np.full(3, Tb[i]), np.tile(Yb[i], (3, 1)), tear=c["tear"], tear_rtol=1e-6, tear_atol=1e-8, tol=1e-8)
            dT.append(float(np.max(np.abs(T / res.T[i] - 1.0))))
        except RuntimeError:
            nfail += 1
    t_ref = time.perf_counter() - t0
    out["numpy_reference"] = {"networks": int(len(idx)), "seconds": t_ref, "networks_per_second": len(idx) / t_ref,
                              "not_converged": nfail, "max_rel_T_difference": max(dT) if dT else None}
    # the drop-in, one network at a time
    from pychemkin_amd.hybridreactornetwork import ReactorNetwork
    from pychemkin_amd.stirreactors import PSR_SetResTime_EnergyConservation as PSR

    def stream(m, T, Y, label=None):
        s = ck.Stream(chem, label=label)
        s.pressure, s.temperature, s.Y, s.mass_flowrate = 10.0 * P_ATM, T, Y, m
        return s

    didx = np.arange(0, n, max(1, n // a.n_dropin))[:a.n_dropin]
    t0, bad = time.perf_counter(), 0
    for i in didx:
        c = cases[i]
        est_mix = ck.Mixture(chem)
        est_mix.pressure, est_mix.temperature, est_mix.Y = 10.0 * P_ATM, float(Tb[i]), Yb[i]
        members = []
        for r in range(3):
            m = PSR(est_mix, label=f"zone {r + 1}")
            m.residence_time = float(c["tau"][r])
            m.steady_state_tolerances = (1e-14, 1e-8)
            m.time_stepping_tolerances = (1e-14, 1e-8)
            for e, s in enumerate(c["ext"][r]):
                m.set_inlet(stream(*s, label=f"in{e}"))
            members.append(m)
        net = ReactorNetwork(chem)
        net.add_reactor_list(members)
        S = c["split"]
        net.add_outflow_connections("zone 1", [("zone 2", 1.0)])
        net.add_outflow_connections("zone 2", [("zone 3", S[1, 2]), ("EXIT>>", S[1, 3])])
        net.add_outflow_connections("zone 3", [("zone 1", S[2, 0]), ("zone 2", S[2, 1]), ("EXIT>>", S[2, 3])])
        net.add_tearingpoint("zone 3")
        bad += net.run() != 0
    torch.cuda.synchronize()
    t_drop = time.perf_counter() - t0
    out["dropin_one_at_a_time"] = {"networks": int(len(didx)), "seconds": t_drop, "networks_per_second": len(didx) / t_drop,
                                   "failed": int(bad)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
