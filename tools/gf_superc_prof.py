"""Seed step of build_gf_superc for one kept state, GFOptions.fused_seeds off and on, same
process and build.

  python tools/gf_superc_prof.py --small          Norb=2, Nbath=2 superc model (Ns=6): a random unit
      vector in sz 0 (924 rows) and its six seeds into sz +1 (792 rows);
  python tools/gf_superc_prof.py --hbm            Norb=1, Nbath=11 (Ns=12): sz 0 -> +1,
      2,704,156 -> 2,496,144 rows, three seeds;
      each: the per-seed chain (edgpu.gf._seed: memset, k_apply_op, k_apply_op_acc, torch.sum,
      divide, host round trip) against one ed_sector_seed_plan call (k_seed_plan + k_seed_scale),
      alternating after a warm-up of each, one hipEvent pair per call, median of --reps (20)
      with min and max beside it, and the bytes the fused call must move over its median;
  python tools/gf_superc_prof.py --build          wall clock of ed_diag's state list ->
      build_gf_superc on the two-orbital superc model of the test suite (Norb=2, Nbath=2, Ns=6),
      fused off and on alternating, median of 5.

Under `rocprofv3 --kernel-trace --stats -- python tools/gf_superc_prof.py ...` the trace holds the
per-launch durations of k_apply_op / k_apply_op_acc / k_seed_plan / k_seed_scale.
"""
import argparse, ctypes, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dmft-ed_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
torch.cuda.init()
from edgpu import _lib, gf  # noqa: E402
from edgpu.diag import DiagOptions, ed_diag  # noqa: E402
from edgpu.gf import GFOptions, build_gf_superc  # noqa: E402
from edgpu.hamiltonian import Sector  # noqa: E402
from edgpu.params import make_config  # noqa: E402


def two_orbital():
    """cases.superc_2orb of the test suite."""
    cfg = make_config(Norb=2, Nbath=2, Nspin=1, ed_mode="superc", Uloc=(2.0, 2.0, 0.0), Ust=1.0, Jh=0.3, Jx=0.3,
                      Jp=0.3, deltasc=0.1, bath="random", seed=19)
    rng = np.random.default_rng(20)
    a = rng.normal(size=(2, 2))
    h = np.zeros((1, 1, 2, 2), dtype=np.complex128)
    h[0, 0] = 0.3 * 0.5 * (a + a.T)
    cfg.impHloc = h
    return cfg


def seed_step(cfg, reps):
    Ns, No, P = cfg.Ns, cfg.Norb, ctypes.c_void_p
    with Sector(cfg, 0, 0, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 1, 0, stored=False, direct=True, real=True) as D:
        x = torch.randn(S.dim, dtype=torch.float64, device="cuda")
        x /= torch.linalg.vector_norm(x)
        # sz + 1: c+_up (op 1) and c_dw (op 0) of every orbital, and their sum
        specs = []
        for a in range(No):
            specs += [[(a, 1, 1)], [(a + Ns, 1, 0)], [(a, 1, 1), (a + Ns, 1, 0)]]
        lev = np.array([l for a in range(No) for l in (a, a + Ns)], dtype=np.int32)
        ops = np.array([1, 0] * No, dtype=np.int32)
        terms = np.array([t for a in range(No) for t in ((2 * a, -1), (2 * a + 1, -1), (2 * a, 2 * a + 1))],
                         dtype=np.int32)
        st = torch.cuda.current_stream()
        print(f"Ns {Ns}: src sz 0 dim {S.dim}, dst sz +1 dim {D.dim}, {len(specs)} seeds, real vectors", flush=True)

        def unfused():
            return [gf._seed(S, D, t[0][2], t, x, False)[1] for t in specs]

        buf = torch.empty((len(specs), D.dim), dtype=torch.float64, device="cuda")
        n2 = np.zeros(len(specs))

        def fused():
            _lib.check(_lib.load().ed_sector_seed_plan(
                S.handle, D.handle, len(lev), P(lev.ctypes.data), P(ops.ctypes.data), len(specs),
                P(terms.ctypes.data), 0, P(x.data_ptr()), P(buf.data_ptr()), P(n2.ctypes.data), P(st.cuda_stream)),
                "ed_sector_seed_plan")
            return list(n2)

        a, b = unfused(), fused()                                   # warm-up of each
        print(f"norm2 fused vs unfused: {max(abs(p - q) / p for p, q in zip(a, b)):.2e}")
        t = {unfused: [], fused: []}
        for r in range(reps):
            for fn in ((unfused, fused) if r % 2 == 0 else (fused, unfused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[fn].append(e0.elapsed_time(e1))                   # ms
        for fn in (unfused, fused):
            print(f"{fn.__name__}: {len(specs)} seeds, hipEvent pair per call, median of {reps}: "
                  f"{statistics.median(t[fn]):.3f} ms (min {min(t[fn]):.3f}, max {max(t[fn]):.3f})", flush=True)
        # what the fused call must move: the target map and the gathered vector once, every seed
        # written by the gather and read and written by the scale
        need = D.dim * 4 + S.dim * 8 + 3 * len(specs) * D.dim * 8
        print(f"fused: {need / 1e6:.1f} MB needed / median = {need / statistics.median(t[fused]) / 1e9:.3f} TB/s "
              f"(whole call: two kernels, the norm2 copy and the host synchronise)", flush=True)


def build(reps):
    cfg = two_orbital()
    _, sl = ed_diag(cfg, DiagOptions())
    opts = {f: GFOptions(fused_seeds=f) for f in (False, True)}
    G = {f: build_gf_superc(cfg, sl, opts[f]) for f in (False, True)}                     # warm-up
    print(f"Ns {cfg.Ns}: {sl.size} kept state(s); fused vs unfused G(iw) "
          f"{np.max(np.abs(G[True][0] - G[False][0])) / np.max(np.abs(G[False][0])):.2e}, F(iw) "
          f"{np.max(np.abs(G[True][2] - G[False][2])) / np.max(np.abs(G[False][0])):.2e}")
    rows = {False: [], True: []}
    for r in range(reps):
        for f in ((False, True) if r % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            build_gf_superc(cfg, sl, opts[f])
            torch.cuda.synchronize()
            rows[f].append(time.perf_counter() - t)
    for f in (False, True):
        print(f"fused_seeds={f}: build_gf_superc (Lmats = Lreal = 5000) wall, median of {reps}: "
              f"{1e3 * statistics.median(rows[f]):.1f} ms (min {1e3 * min(rows[f]):.1f}, max {1e3 * max(rows[f]):.1f})",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--hbm", action="store_true")
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.small:
        seed_step(make_config(Norb=2, Nbath=2, ed_mode="superc", deltasc=0.2, bath="random", seed=3), a.reps)
    if a.hbm:
        seed_step(make_config(Norb=1, Nbath=11, ed_mode="superc", deltasc=0.2), a.reps)
    if a.build:
        build(5)
