"""Seed step of build_chi for one kept state: one ed_sector_seed_diag call (k_seed_diag +
k_seed_scale) against what can be done without it for the same seeds, a torch elementwise chain
(per seed: one precomputed weight tensor times the vector, one norm with its host round trip, one
scale), in the same process and build.

  python tools/chi_prof.py            the Nlevels = 28 (7,7) sector (Norb=2, Nbath=6: Ns = 14,
      direct build, 11,778,624 rows), a random unit vector, the three-orbital seed table over six
      levels (two impurity orbitals and one bath level standing in for the third): 4 real seeds
      (the spin part), 11 real seeds and 11 complex seeds;
  python tools/chi_prof.py --small    the same on the (4,5) sector of Norb=2, Nbath=4 (52,920 rows).

Kernel and chain alternate after a warm-up of each, one device-event pair per call, median of
--reps (20) with min and max beside it.  Each time is printed beside the kernel's own byte model:
(4 + sizeof(val)) * dim read, nseed * sizeof(val) * dim written, and the scale pass
2 * nseed * sizeof(val) * dim; and beside the chain's: per seed 8 * dim (weights) +
sizeof(val) * dim read and sizeof(val) * dim written, sizeof(val) * dim for the norm, and
2 * sizeof(val) * dim for the scale.  A manual tool: no test runs it.
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dmft-ed_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
torch.cuda.init()
from edgpu import chi  # noqa: E402
from edgpu.hamiltonian import Sector  # noqa: E402
from edgpu.params import make_config  # noqa: E402


def run(cfg, q, reps):
    Ns = cfg.Ns
    levels = [0, 1, 2, Ns, Ns + 1, Ns + 2]
    table = chi.seed_table(make_config(Norb=3, Nbath=1))            # 11 seeds over six levels
    rows = []
    with Sector(cfg, q[0], q[1], stored=False, direct=True, real=True) as S:
        hmap = torch.from_numpy(S.map().astype(np.int64)).cuda()
        for label, part, cplx in (("4 real", table[:4], False), ("11 real", table, False), ("11 complex", table, True)):
            dt = torch.complex128 if cplx else torch.float64
            vs, ns, dim = (16 if cplx else 8), len(part), S.dim
            x = torch.randn(dim, dtype=dt, device="cuda")
            x /= torch.linalg.vector_norm(x)
            w = np.array([t[2] for t in part])
            # the chain's weight tensors: the row factor of every seed, precomputed (not timed)
            fac = torch.zeros((ns, dim), dtype=torch.float64, device="cuda")
            for l, lv in enumerate(levels):
                b = ((hmap >> lv) & 1).to(torch.float64)
                for s in range(ns):
                    fac[s] += float(w[s, l]) * b
            out = torch.empty((ns, dim), dtype=dt, device="cuda")
            ybuf = torch.empty((ns, dim), dtype=dt, device="cuda")

            def kernel():
                return S.seed_diag(x, levels, w, out=out)[1]

            def chain():
                n2 = []
                for s in range(ns):
                    torch.mul(fac[s], x, out=ybuf[s])
                    n2.append(float(torch.vdot(ybuf[s], ybuf[s]).real.item()))
                    if n2[-1] > 0:
                        ybuf[s].mul_(1.0 / np.sqrt(n2[-1]))
                return n2

            a, b = kernel(), chain()                                 # warm-up of each
            dn = max(abs(p - r) / r for p, r in zip(a, b) if r > 0)
            dv = float(torch.max(torch.abs(out - ybuf)).item())
            t = {kernel: [], chain: []}
            for r in range(reps):
                for fn in ((kernel, chain) if r % 2 == 0 else (chain, kernel)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    t[fn].append(e0.elapsed_time(e1))                # ms
            need_k = (4 + vs) * dim + ns * vs * dim + 2 * ns * vs * dim
            need_c = ns * ((8 + vs) * dim + vs * dim + vs * dim + 2 * vs * dim)
            row = dict(case=label, dim=dim, nseed=ns, reps=reps, norm2_rel=dn, seeds_abs=dv)
            for fn, need in ((kernel, need_k), (chain, need_c)):
                med = statistics.median(t[fn])
                row[fn.__name__] = dict(median_ms=med, min_ms=min(t[fn]), max_ms=max(t[fn]), model_mb=need / 1e6,
                                        model_tb_s=need / med / 1e9)
                print(f"{label}, dim {dim}: {fn.__name__}: device-event pair per call, median of {reps}: {med:.3f} ms "
                      f"(min {min(t[fn]):.3f}, max {max(t[fn]):.3f}); byte model {need / 1e6:.1f} MB -> "
                      f"{need / med / 1e9:.3f} TB/s over the whole call", flush=True)
            print(f"{label}: kernel vs chain norm2 {dn:.2e}, seeds {dv:.2e}", flush=True)
            rows.append(row)
            del x, fac, out, ybuf
            torch.cuda.empty_cache()
    print(json.dumps(dict(tool="chi_prof", sector=list(q), rows=rows)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.small:
        run(make_config(Norb=2, Nbath=4), (4, 5), a.reps)
    else:
        run(make_config(Norb=2, Nbath=6), (7, 7), a.reps)
