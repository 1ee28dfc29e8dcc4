"""Pair seed step of build_chi(pair=True) for one kept state: one ed_sector_seed_pair call
(k_seed_pair + k_seed_scale) against the unfused chain through the intermediate sector for the same
seeds (per seed: ed_sector_apply_op into the intermediate sector, a memset of the target row,
ed_sector_apply_op_acc into it, one dot with its host round trip, one scale), in the same process and
build.

  python tools/chi_pair_prof.py           Norb=2, Nbath=6 (Ns = 14, direct builds): the kept state in
      (7,7) (11,778,624 rows), the Delta_a^+ seeds of both orbitals into (8,8) (9,018,009 rows) through
      (8,7) (10,306,296 rows); a real and a complex random unit vector;
  python tools/chi_pair_prof.py --small   the same on Norb=2, Nbath=4: (4,5) -> (5,6) through (5,5).

Kernel and chain alternate after a warm-up of each, one device-event pair per call, median of --reps
(20) with min and max beside it.  Byte models, with v = sizeof(val), ds / dm / dd the rows of the
source, intermediate and target sectors and n the seeds: kernel 4 dd (map) + n v dd (gathered vector
elements, at most) + n v dd written + 2 n v dd for the scale pass; chain, per seed, v dm (memset) +
(4 + v) ds + v dm (apply_op: map and vector read, scattered writes) + v dd (memset) + (4 + v) dm + 2 v dd
(apply_op_acc: read-modify-write) + v dd (dot) + 2 v dd (scale).  A manual tool: no test runs it.
"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dmft-ed_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
torch.cuda.init()
from edgpu import _lib  # noqa: E402
from edgpu.hamiltonian import Sector  # noqa: E402
from edgpu.params import make_config  # noqa: E402

P = ctypes.c_void_p


def run(cfg, q, reps):
    Ns, No = cfg.Ns, cfg.Norb
    images = [(a, 1, a + Ns, 1) for a in range(No)]                # c^+ on (a, up), then c^+ on (a, dw)
    terms = [(a, -1) for a in range(No)]
    rows = []
    L = _lib.load()
    with Sector(cfg, q[0], q[1], stored=False, direct=True, real=True) as S, \
            Sector(cfg, q[0] + 1, q[1], stored=False, direct=True, real=True) as M, \
            Sector(cfg, q[0] + 1, q[1] + 1, stored=False, direct=True, real=True) as D:
        ds, dm, dd, n = S.dim, M.dim, D.dim, len(terms)
        for label, cplx in (("%d real" % n, False), ("%d complex" % n, True)):
            dt = torch.complex128 if cplx else torch.float64
            vs, vt = (16 if cplx else 8), (1 if cplx else 0)
            x = torch.randn(ds, dtype=dt, device="cuda")
            x /= torch.linalg.vector_norm(x)
            out = torch.empty((n, dd), dtype=dt, device="cuda")
            ybuf = torch.empty((n, dd), dtype=dt, device="cuda")
            mid = torch.empty(dm, dtype=dt, device="cuda")
            st = P(torch.cuda.current_stream().cuda_stream)

            def kernel():
                return S.seed_pair(x, D, images, terms, out=out)[1]

            def chain():
                n2 = []
                for s, (lev1, op1, lev2, op2) in enumerate(images):
                    _lib.check(L.ed_sector_apply_op(S.handle, M.handle, op1, lev1, vt, P(x.data_ptr()), P(mid.data_ptr()), st),
                               "apply_op")
                    ybuf[s].zero_()
                    _lib.check(L.ed_sector_apply_op_acc(M.handle, D.handle, op2, lev2, 1.0, 0.0, vt, P(mid.data_ptr()),
                                                        P(ybuf[s].data_ptr()), st), "apply_op_acc")
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
            need_k = 4 * dd + n * vs * dd + n * vs * dd + 2 * n * vs * dd
            need_c = n * (vs * dm + (4 + vs) * ds + vs * dm + vs * dd + (4 + vs) * dm + 2 * vs * dd + vs * dd + 2 * vs * dd)
            row = dict(case=label, dims=[ds, dm, dd], nseed=n, reps=reps, norm2_rel=dn, seeds_abs=dv)
            for fn, need in ((kernel, need_k), (chain, need_c)):
                med = statistics.median(t[fn])
                row[fn.__name__] = dict(median_ms=med, min_ms=min(t[fn]), max_ms=max(t[fn]), model_mb=need / 1e6,
                                        model_tb_s=need / med / 1e9)
                print(f"{label}, rows {ds} -> {dm} -> {dd}: {fn.__name__}: device-event pair per call, median of {reps}: "
                      f"{med:.3f} ms (min {min(t[fn]):.3f}, max {max(t[fn]):.3f}); byte model {need / 1e6:.1f} MB -> "
                      f"{need / med / 1e9:.3f} TB/s over the whole call", flush=True)
            row["time_ratio"] = row["kernel"]["median_ms"] / row["chain"]["median_ms"]
            row["byte_ratio"] = need_k / need_c
            print(f"{label}: kernel / chain time {row['time_ratio']:.3f}, bytes {row['byte_ratio']:.3f}; norm2 {dn:.2e}, "
                  f"seeds {dv:.2e}", flush=True)
            rows.append(row)
            del x, out, ybuf, mid
            torch.cuda.empty_cache()
    print(json.dumps(dict(tool="chi_pair_prof", sector=list(q), rows=rows)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.small:
        run(make_config(Norb=2, Nbath=4), (4, 5), a.reps)
    else:
        run(make_config(Norb=2, Nbath=6), (7, 7), a.reps)
