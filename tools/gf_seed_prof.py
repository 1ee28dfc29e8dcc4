"""Seed step of build_gf with GFOptions.fused_seeds off and on, same process and build.

  python tools/gf_seed_prof.py --nbath 5          hybrid Norb=3 model: ed_diag, then build_gf
      (orbital-mixed seeds, batched persistent Lanczos) fused off / on in alternating order
      after a warm-up of each; prints per-run wall times of build_gf, the time inside the seed
      step (edgpu.gf._seed / _fused_seeds, both synchronous) and its share; --modes lists the
      persistent mode (ed_sector_lanc_mode, -1: multi-kernel path) of the largest sector for
      Nbath = 2..8 instead.
  python tools/gf_seed_prof.py --hbm 11           seed step alone at an HBM-sized sector:
      Norb=3, Ns=3+11, a random unit vector in (Ns/2, Ns/2) and its 9 c+ seeds (3 single,
      3 real pairs, 3 complex pairs) into (Ns/2+1, Ns/2), per-seed chain against two
      ed_sector_seed_batch calls.

Under `rocprofv3 --kernel-trace --stats -- python tools/gf_seed_prof.py ...` the trace holds the
per-launch durations of k_apply_op / k_apply_op_acc / k_seed_gather / k_seed_scale.
"""
import argparse, ctypes, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dmft-ed_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
torch.cuda.init()
from edgpu import _lib, gf  # noqa: E402
from edgpu.diag import DiagOptions, ed_diag  # noqa: E402
from edgpu.gf import GFOptions, build_gf  # noqa: E402
from edgpu.hamiltonian import Sector  # noqa: E402
from edgpu.params import make_config  # noqa: E402
from edgpu.sectors import setup_pointers  # noqa: E402


def model(nbath):
    cfg = make_config(Norb=3, Nbath=nbath, Nspin=2, bath_type="hybrid", Uloc=(2.0, 1.8, 1.6), Ust=1.0, Jh=0.2,
                      xmu=0.3, bath="random", seed=21)
    rng = np.random.default_rng(22)
    h = np.zeros((2, 2, 3, 3), dtype=np.complex128)
    for s in range(2):
        a = rng.normal(size=(3, 3))
        h[s, s] = 0.15 * (a + a.T)
    cfg.impHloc = h
    return cfg


class Clock:
    """Wall time spent inside the (synchronous) seed functions of edgpu.gf."""

    def __init__(self):
        self.t = 0.0
        for name in ("_seed", "_fused_seeds"):
            setattr(gf, name, self.wrap(getattr(gf, name)))

    def wrap(self, fn):
        def inner(*a, **k):
            t = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t += time.perf_counter() - t
        return inner


def modes():
    for nb in range(2, 9):
        cfg = model(nb)
        big = max(setup_pointers(cfg), key=lambda s: s.dim)
        with Sector(cfg, big.q1, big.q2, stored=True, real=True) as S:
            m = [_lib.load().ed_sector_lanc_mode(S.handle, vt, -1) for vt in (0, 1)]
        print(f"Nbath {nb} Ns {cfg.Ns}: largest sector ({big.q1},{big.q2}) dim {big.dim}: persistent mode real {m[0]} "
              f"complex {m[1]}", flush=True)


def small(nbath, reps):
    cfg = model(nbath)
    t = time.perf_counter()
    _, sl = ed_diag(cfg, DiagOptions())
    secs = setup_pointers(cfg)
    print(f"Ns {cfg.Ns}: ed_diag {time.perf_counter() - t:.1f} s, ground states in "
          f"{[(secs[i - 1].q1, secs[i - 1].q2, secs[i - 1].dim) for i in sl.sectors]}", flush=True)
    clock = Clock()
    opts = {f: GFOptions(fused_seeds=f) for f in (False, True)}
    G = {}
    for f in (False, True):                       # warm-up: sector builds cached nowhere, kernels loaded
        G[f] = build_gf(cfg, sl, opts[f])
    print(f"fused vs unfused G(iw): {np.max(np.abs(G[True][0] - G[False][0])) / np.max(np.abs(G[False][0])):.2e}")
    rows = {False: [], True: []}
    for r in range(reps):
        for f in ((False, True) if r % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            clock.t = 0.0
            t = time.perf_counter()
            build_gf(cfg, sl, opts[f])
            rows[f].append((time.perf_counter() - t, clock.t))
    for f in (False, True):
        tot, seed = [x[0] for x in rows[f]], [x[1] for x in rows[f]]
        print(f"fused_seeds={f}: build_gf median {1e3 * statistics.median(tot):.1f} ms (min {1e3 * min(tot):.1f}, "
              f"max {1e3 * max(tot):.1f}); seed step median {1e3 * statistics.median(seed):.1f} ms "
              f"(min {1e3 * min(seed):.1f}, max {1e3 * max(seed):.1f}); share "
              f"{100 * statistics.median(seed) / statistics.median(tot):.1f} %", flush=True)


def hbm(nbath, reps):
    cfg = model(nbath)
    Ns, P = cfg.Ns, ctypes.c_void_p
    n = Ns // 2
    with Sector(cfg, n, n, stored=False, direct=True, real=True) as S, \
            Sector(cfg, n + 1, n, stored=False, direct=True, real=True) as D:
        print(f"Ns {Ns}: src ({n},{n}) dim {S.dim}, dst ({n + 1},{n}) dim {D.dim}", flush=True)
        x = torch.randn(S.dim, dtype=torch.float64, device="cuda")
        x /= torch.linalg.vector_norm(x)
        xc = x.to(torch.complex128)
        singles = [[(a, 1)] for a in range(3)]
        real2 = [[(a, 1), (b, 1)] for a in range(3) for b in range(a + 1, 3)]
        cplx2 = [[(a, 1), (b, 1j)] for a in range(3) for b in range(a + 1, 3)]
        st = torch.cuda.current_stream()

        def unfused():
            out = [gf._seed(S, D, 1, t, x, False) for t in singles + real2]
            out += [gf._seed(S, D, 1, t, xc, True) for t in cplx2]
            return [o[1] for o in out]

        def fused():
            norms = []
            for vec, terms, dt in ((x, singles + real2, torch.float64), (xc, cplx2, torch.complex128)):
                coef = np.zeros((len(terms), 3), dtype=np.complex128)
                for q, t in enumerate(terms):
                    for lv, c in t:
                        coef[q, lv] = c
                lev = np.arange(3, dtype=np.int32)
                buf = torch.empty((len(terms), D.dim), dtype=dt, device="cuda")
                n2 = np.zeros(len(terms))
                _lib.check(_lib.load().ed_sector_seed_batch(
                    S.handle, D.handle, 1, 3, P(lev.ctypes.data), len(terms), P(coef.ctypes.data),
                    0 if dt == torch.float64 else 1, P(vec.data_ptr()), P(buf.data_ptr()), P(n2.ctypes.data),
                    P(st.cuda_stream)), "ed_sector_seed_batch")
                norms += list(n2)
            return norms

        a, b = unfused(), fused()                                   # warm-up
        print(f"norm2 fused vs unfused: {max(abs(p - q) / p for p, q in zip(a, b)):.2e}")
        t = {unfused: [], fused: []}
        for r in range(reps):
            for fn in ((unfused, fused) if r % 2 == 0 else (fused, unfused)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[fn].append(time.perf_counter() - t0)
        for fn in (unfused, fused):
            print(f"{fn.__name__}: 9 seeds, median {1e3 * statistics.median(t[fn]):.1f} ms (min {1e3 * min(t[fn]):.1f}, "
                  f"max {1e3 * max(t[fn]):.1f})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbath", type=int)
    ap.add_argument("--hbm", type=int)
    ap.add_argument("--modes", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.modes:
        modes()
    if a.nbath:
        small(a.nbath, a.reps)
    if a.hbm:
        hbm(a.hbm, a.reps)
