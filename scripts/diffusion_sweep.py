"""Time the three batched diffusion kernels on one GPU and write profiles/diffusion_sweep.json.

GRI-3.0 CH4/air on a phi x T x P grid between the fresh mixture and its complete-combustion products (a progress
variable runs with T), every species of the mechanism present at a trace level so that no state is special:
binary D_jk [n][53][53], mixture-averaged D_km [53][n] and the ordinary multicomponent D_ij [n][53][53].  Each
kernel is timed with device events after a warm-up launch; the inputs and the output buffers are on the device
before the clock starts.  The numpy restatement of tests/diffusion_reference.py evaluates a sample of each sweep
on one host core, for the cost of a CPU evaluation and a cross-check.  The rates are reported, not gated.

    python scripts/diffusion_sweep.py [--log2-n 20] [--log2-matrix 17] [--repeats 5] [--out profiles/diffusion_sweep.json]
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


def grid(mech, log2n):
    """T [n], P [n], Y [KK][n]: phi in [0.5, 2], T in [300, 3000] K, P in [0.1, 100] atm."""
    k = (log2n + 1) // 3
    n_phi, n_T, n_P = 1 << (log2n - 2 * k), 1 << k, 1 << k
    g = np.stack(np.meshgrid(np.linspace(0.5, 2.0, n_phi), np.linspace(300.0, 3000.0, n_T),
                             P_ATM * np.logspace(-1.0, 2.0, n_P), indexing="ij"), axis=-1).reshape(-1, 3)
    phi, T, P = g[:, 0], g[:, 1], g[:, 2]
    c = (T - 300.0) / 2700.0  # progress: fresh at 300 K, burnt at 3000 K
    sp = mech.species.index
    X = np.full((g.shape[0], mech.KK), 1e-7)
    burn = np.minimum(phi, 1.0) * c  # CH4 burnt per 2 O2 supplied
    X[:, sp("CH4")] += phi - burn
    X[:, sp("O2")] += 2.0 - 2.0 * burn
    X[:, sp("CO2")] += burn
    X[:, sp("H2O")] += 2.0 * burn
    X[:, sp("N2")] += 2.0 * 0.79 / 0.21
    Y = X * mech.wt
    Y /= Y.sum(axis=1, keepdims=True)
    return T.copy(), P.copy(), np.ascontiguousarray(Y.T), dict(phi=[0.5, 2.0, n_phi], T_K=[300.0, 3000.0, n_T],
                                                               P_atm=[0.1, 100.0, n_P])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=20, help="states of the mixture-averaged sweep")
    ap.add_argument("--log2-matrix", type=int, default=17, help="states of the two sweeps with [n][KK][KK] output")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-ref", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_sweep.json"))
    a = ap.parse_args()

    import torch

    import diffusion_reference as dr
    from pychemkin_amd import _native, transport
    from pychemkin_amd.mechanism import Mechanism

    mech = Mechanism.from_files(os.path.join(ROOT, "data", "grimech30_chem.inp"),
                                os.path.join(ROOT, "data", "grimech30_thermo.dat"))
    with open(os.path.join(ROOT, "data", "grimech30_transport.dat")) as f:
        params = transport.species_params(transport.parse_transport_text(f.read()), mech.species)
    fits = transport.diffusion_fits(mech.wt, params)
    dm = _native.DeviceMechanism(mech.to_tables(), device=0)
    dt = _native.DeviceTransport(dm, transport.viscosity_fits(mech.wt, params), None, fits)
    KK = mech.KK
    lib = _native.lib()
    stream = _native._stream_ptr(dm.device)

    def launch(kind, n, Td, Pd, Yd, out, info):
        if kind == "binary":
            rc = lib.ckmi_binary_diffusion(dt._h, n, Td.data_ptr(), Pd.data_ptr(), out.data_ptr(), stream)
        elif kind == "mixture_averaged":
            rc = lib.ckmi_mixture_diffusion(dt._h, n, Td.data_ptr(), Pd.data_ptr(), Yd.data_ptr(), out.data_ptr(), stream)
        else:
            rc = lib.ckmi_multicomponent_diffusion(dt._h, n, Td.data_ptr(), Pd.data_ptr(), Yd.data_ptr(), out.data_ptr(),
                                                   info.data_ptr(), stream)
        assert rc == 0, lib.ckmi_last_error()

    def reference(kind, T, P, Y):
        if kind == "binary":
            return dr.binary_from_fits(T, P, fits)
        if kind == "mixture_averaged":
            return dr.mixture_averaged(T, P, Y, mech.wt, fits)
        return dr.multicomponent(T, P, Y, mech.wt, fits)

    res = {"what": "batched diffusion coefficients, GRI-3.0 CH4/air, phi x T x P grid, one GPU",
           "device": torch.cuda.get_device_name(0), "KK": KK, "sweeps": {}}
    for kind, log2n in (("binary", a.log2_matrix), ("mixture_averaged", a.log2_n), ("multicomponent", a.log2_matrix)):
        T, P, Y, g = grid(mech, log2n)
        n = T.size
        Td, Pd, Yd = dm._dev(T), dm._dev(P), dm._dev(Y)
        shape = (KK, n) if kind == "mixture_averaged" else (n, KK, KK)
        out = torch.empty(shape, dtype=torch.float64, device=dm.device)
        info = torch.zeros(n, dtype=torch.int32, device=dm.device)
        launch(kind, n, Td, Pd, Yd, out, info)  # warm-up: module load
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(kind, n, Td, Pd, Yd, out, info)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        idx = np.arange(0, n, max(1, n // a.n_ref))[:a.n_ref]
        t0 = time.perf_counter()
        ref = reference(kind, T[idx], P[idx], np.ascontiguousarray(Y[:, idx]))
        t_ref = time.perf_counter() - t0
        ii = torch.as_tensor(idx, device=dm.device)
        got = (out[:, ii] if kind == "mixture_averaged" else out[ii]).cpu().numpy()
        if kind == "multicomponent":
            diff = float(np.max(np.abs(got - ref).reshape(idx.size, -1).max(axis=1) / np.abs(ref).reshape(idx.size, -1).max(axis=1)))
        else:
            diff = float(np.max(np.abs(got / ref - 1)))
        med = float(np.median(ms))
        s = {"states": n, "grid": g, "milliseconds": ms, "milliseconds_median": med,
             "states_per_second": n / med * 1e3, "output_bytes_per_state": int(np.prod(shape) // n * 8),
             "output_GB_per_second": float(np.prod(shape)) * 8 / med * 1e-6,
             "nonzero_info": int(torch.count_nonzero(info).item()),
             "numpy_reference": {"states": int(idx.size), "seconds": t_ref, "states_per_second": idx.size / t_ref,
                                 "max_difference": diff,
                                 "difference_is": ("max |D - ref| / max |ref| per state" if kind == "multicomponent"
                                                   else "max |D / ref - 1|")}}
        res["sweeps"][kind] = s
        print(kind, json.dumps(s), flush=True)
        del Td, Pd, Yd, out, info
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
