"""Timing of build_sigma (ed_sigma_build, k_sigma<N>) at Lmats = Lreal = 5000
for a model of n = 1 blocks and one with a single n = 6 block, against the
same work with numpy.linalg.inv on the host, alternating in one process after
a warm-up of each: median of 20 with the range.

  device   G and Sigma stay in HBM (torch tensors in, device_out=True); wall
           time of the call plus a stream synchronise
  roundtrip numpy arrays in and out (upload, launch, ten downloads)
  numpy    Delta from the same pole table, invG0, two numpy.linalg.inv per
           point (batched over the grid) and the difference

    python tools/sigma_prof.py [--runs 20] [--L 5000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dmft-ed_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def models():
    from edgpu.params import make_config

    n1 = make_config(Norb=3, Nbath=4, Nspin=2, bath="random", seed=3)                       # six blocks of n = 1
    n6 = make_config(Norb=3, Nbath=4, Nspin=2, ed_mode="nonsu2", bath_type="hybrid", bath="random", seed=4)
    rng = np.random.default_rng(6)
    a = rng.normal(size=(6, 6)) + 1j * rng.normal(size=(6, 6))
    n6.impHloc = (0.15 * (a + a.conj().T)).reshape(2, 3, 2, 3).transpose(0, 2, 1, 3).copy()  # one block of n = 6
    return {"n=1 x 6 blocks": n1, "n=6 x 1 block": n6}


def numpy_sigma(blocks, norb, shape, zs, G):
    out = []
    for z, g in zip(zs, G):
        S = np.zeros(shape + (len(z),), dtype=np.complex128)
        for B in blocks:
            n = len(B.idx)
            D = np.einsum("p,pi,pj,pl->lij", B.c, B.w, np.conj(B.w), 1.0 / (z[None, :] - B.e[:, None]))
            i0 = z[:, None, None] * np.eye(n)[None] - B.h[None] - D
            at = [(i // norb, j // norb, i % norb, j % norb) for i in B.idx for j in B.idx]
            Gb = np.array([g[a] for a in at]).reshape(n, n, -1).transpose(2, 0, 1)
            s = i0 - np.linalg.inv(Gb)
            np.linalg.inv(i0)                                                                # G0, as the device call
            for k, a in enumerate(at):
                S[a] = s[:, k // n, k % n]
        out.append(S)
    return out


def main():
    import torch

    from edgpu.gf import GFOptions, matsubara, realaxis
    from edgpu.sigma import bath_functions, build_sigma, sigma_blocks

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--L", type=int, default=5000)
    a = ap.parse_args()
    g = GFOptions(Lmats=a.L, Lreal=a.L, beta=50.0, eps=0.05)
    zs = (1j * matsubara(g.beta, a.L), realaxis(g.wini, g.wfin, a.L) + 1j * g.eps)
    rows = {}
    for name, cfg in models().items():
        blocks = sigma_blocks(cfg)
        shape = (cfg.Nspin, cfg.Nspin, cfg.Norb, cfg.Norb)
        bf = bath_functions(cfg, g)
        # a physical G: the bath's G0 dressed with a one-pole self-energy on every block
        G = []
        for z, g0 in zip(zs, (bf.G0mats, bf.G0real)):
            arr = np.zeros_like(g0)
            for B in blocks:
                n = len(B.idx)
                at = [(i // cfg.Norb, j // cfg.Norb, i % cfg.Norb, j % cfg.Norb) for i in B.idx for j in B.idx]
                m = np.array([g0[x] for x in at]).reshape(n, n, -1).transpose(2, 0, 1)
                gi = np.linalg.inv(np.linalg.inv(m) - (0.5 / (z - 0.3))[:, None, None] * np.eye(n)[None])
                for k, x in enumerate(at):
                    arr[x] = gi[:, k // n, k % n]
            G.append(arr)
        Gd = [torch.from_numpy(x).cuda() for x in G]

        def device():
            build_sigma(cfg, Gd[0], Gd[1], g, device_out=True)
            torch.cuda.synchronize()

        def roundtrip():
            return build_sigma(cfg, G[0], G[1], g)

        def host():
            return numpy_sigma(blocks, cfg.Norb, shape, zs, G)

        ref, got = host(), roundtrip()
        dist = max(np.max(np.abs(r - s)) for r, s in zip(ref, (got.Smats, got.Sreal)))
        paths = {"device": device, "roundtrip": roundtrip, "numpy": host}
        for f in paths.values():
            f()
        t = {k: [] for k in paths}
        for _ in range(a.runs):
            for k, f in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
        rows[name] = {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in t.items()}
        rows[name]["max_abs_sigma_diff"] = float(dist)
        print(name, json.dumps(rows[name]))
    print(json.dumps({"sigma_prof": rows, "L": a.L, "runs": a.runs}))


if __name__ == "__main__":
    main()
