"""Lockstep multi-vector Lanczos (ed_sector_lanc_tridiag_lockstep) against the same seeds through
ed_sector_lanc_tridiag_batch on the same sector object, which runs them one after the other (the
sector is built with ED_OPT_NO_PERSIST where it would otherwise fit the persistent kernel), in one
process and one build.

  python tools/lockstep_prof.py           Norb=1, Nbath=13 (Nlevels = 28): the target sector (8,7) of the
      (7,7) ground state, stored (10,306,296 rows); the (6,6) sector of Nbath=11 (853,776 rows) and the (5,5)
      sector of Nbath=9 (63,504 rows) between the ends; and hybrid Norb=3, Nbath=5 (Ns = 8), sector (2,4),
      1,960 rows with ED_OPT_NO_PERSIST: the launch-bound end;
  python tools/lockstep_prof.py --small   only the last.

For k in 1, 2, 4, 8 random unit seeds, real and complex: 32 Lanczos steps (--steps) per call, threshold
0 (no run stops).  The two entries alternate after a warm-up of each, one device-event pair per
call, median of --reps (10) with min and max beside it.  Both entries return with the stream idle, so
a pair spans the whole call: workspace allocation, the start pass, the steps, the download of alpha
and beta.  Byte models per Krylov step, with v = sizeof(val), W the bytes of the stored matrix stream
(4 per slot packed, 4 + sizeof(H) plain, + sizeof(H) per row for the diagonal) and d the rows:
sequential k (W + 6 v d) (H·v reads R, P and writes P, W; part B reads W, P and writes R, when the one-pass
kernel serves; the gathers are not counted), lockstep W + 6 k v d.  A manual tool: no test runs it.
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dmft-ed_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
torch.cuda.init()
from edgpu.gf import _tridiag_batch  # noqa: E402
from edgpu.hamiltonian import Sector  # noqa: E402
from edgpu.params import make_config  # noqa: E402


def run(name, cfg, q, options, steps, reps, checks):
    rows = []
    with Sector(cfg, q[0], q[1], stored=True, real=True, options=options) as S:
        d, info = S.dim, S.info
        hs = 8
        W = int(info.padded) * (4 if info.packed else 4 + hs) + d * hs
        print(f"{name}: sector {q}, {d} rows, nnz {S.nnz}, {'packed' if info.packed else 'plain SELL'}, matrix stream "
              f"{W / 1e6:.1f} MB, options {options}", flush=True)
        # the block kernel at this size (XCD remap from 1024 blocks, non-temporal matrix loads beyond 192 MB)
        # against the one-pass kernel, column by column
        S.set_options(*options, "stored_exact")
        for cplx, nv in ((False, 8), (False, 2), (True, 4), (True, 1)):
            X = torch.randn((d, nv), dtype=torch.complex128 if cplx else torch.float64, device="cuda")
            Y = S.hxv_multi(X)
            same = True
            for v in range(nv):
                col, ref = X[:, v].contiguous(), torch.empty(d, dtype=X.dtype, device="cuda")
                S.hxv_dev(col, ref)
                same = same and bool(torch.equal(Y[:, v].contiguous().view(torch.float64), ref.view(torch.float64)))
            torch.cuda.synchronize()
            print(f"{name}: hxv_multi, {'complex' if cplx else 'real'} nvec={nv}, grid of {(d + 255) // 256} blocks, matrix "
                  f"{W / 1e6:.0f} MB: {'bit-identical to' if same else 'DIFFERS from'} the one-pass H·v", flush=True)
            checks.append(dict(case=name, vectors="complex" if cplx else "real", nvec=nv, bit_identical=same))
            del X, Y
        S.set_options(*options)
        torch.cuda.empty_cache()
        for cplx in (False, True):
            assert S.lanc_mode(real=not cplx) < 0, "the batch entry must run the seeds one after the other here"
            vs = 16 if cplx else 8
            for k in (1, 2, 4, 8):
                seeds = torch.randn((k, d), dtype=torch.complex128 if cplx else torch.float64, device="cuda")
                seeds /= torch.linalg.vector_norm(seeds, dim=1, keepdim=True)
                torch.cuda.synchronize()

                def lockstep():
                    return S.lanc_tridiag_lockstep(seeds, steps, 0.0)

                def sequential():
                    return _tridiag_batch(S, seeds, steps, not cplx, 0.0)

                (a1, b1, _), (a0, b0, _) = lockstep(), sequential()          # warm-up of each
                n8 = min(8, steps)
                scale = np.max(np.abs(a0)) + 2 * np.max(np.abs(b0))
                d8 = max(np.max(np.abs(a1[:, :n8] - a0[:, :n8])), np.max(np.abs(b1[:, :n8] - b0[:, :n8]))) / scale
                dall = max(np.max(np.abs(a1 - a0)), np.max(np.abs(b1 - b0))) / scale
                t = {lockstep: [], sequential: []}
                for r in range(reps):
                    for fn in ((lockstep, sequential) if r % 2 == 0 else (sequential, lockstep)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        t[fn].append(e0.elapsed_time(e1))                    # ms
                need = {lockstep: steps * (W + 6 * k * vs * d), sequential: steps * k * (W + 6 * vs * d)}
                row = dict(case=name, vectors="complex" if cplx else "real", k=k, steps=steps, reps=reps,
                           first8_rel=d8, all_steps_rel=dall)
                for fn in (lockstep, sequential):
                    med = statistics.median(t[fn])
                    row[fn.__name__] = dict(median_ms=med, min_ms=min(t[fn]), max_ms=max(t[fn]), model_mb=need[fn] / 1e6,
                                            model_tb_s=need[fn] / med / 1e9)
                    print(f"{name} {row['vectors']} k={k}: {fn.__name__}: {steps} steps, device-event pair per call, median "
                          f"of {reps}: {med:.3f} ms (min {min(t[fn]):.3f}, max {max(t[fn]):.3f}); byte model "
                          f"{need[fn] / 1e6:.1f} MB -> {need[fn] / med / 1e9:.3f} TB/s over the whole call", flush=True)
                row["time_ratio"] = row["lockstep"]["median_ms"] / row["sequential"]["median_ms"]
                row["byte_ratio"] = need[lockstep] / need[sequential]
                print(f"{name} {row['vectors']} k={k}: lockstep / sequential time {row['time_ratio']:.3f}, bytes "
                      f"{row['byte_ratio']:.3f}; alpha, beta: first 8 steps {d8:.2e}, all {steps} steps {dall:.2e}", flush=True)
                rows.append(row)
                del seeds
                torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=32)
    a = ap.parse_args()
    out, checks = [], []
    if not a.small:
        out += run("N28", make_config(Norb=1, Nbath=13, bath="random", seed=20251015), (8, 7), (), a.steps, a.reps, checks)
        # two sizes between the ends: where the complex runs change sides
        out += run("N24", make_config(Norb=1, Nbath=11, bath="random", seed=20251015), (6, 6), (), a.steps, a.reps, checks)
        out += run("N20", make_config(Norb=1, Nbath=9, bath="random", seed=20251015), (5, 5), (), a.steps, a.reps, checks)
    out += run("H3", make_config(Norb=3, Nbath=5, Nspin=1, bath_type="hybrid", Uloc=(2.0, 2.0, 2.0), Ust=1.0, Jh=0.2,
                                 bath="random", seed=5), (2, 4), ("no_persist",), a.steps, a.reps, checks)
    print(json.dumps(dict(tool="lockstep_prof", hxv_multi=checks, rows=out)))
