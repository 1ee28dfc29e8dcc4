"""Twin-sector measurements on one MI355X.

  1. ed_sector_twin_vector on configs[3]'s largest asymmetric sector,
     (6,5) -> (5,6) (731,808 rows): the tiled transpose against the forced
     gather (ED_OPT_TWIN_GATHER), real and complex vectors; hipEvent pairs
     around 50 back-to-back calls each (one call is a few microseconds, less
     than a launch), median of 20 pairs after 5 warm-up pairs, alternating
     kernels; the fraction of 8 TB/s on the bytes read + written (16 or 32
     bytes per row; the 6 and 12 MB vectors stay in the caches, so this is
     not an HBM figure).
  2. configs[3] farm_diag wall time with ed_twin off and on (91 of the 169
     sectors), alternating runs in one process, median of `--runs` each; the
     ed_twin-off figure stands beside profiles/farm_c4_1gpu.json.

Usage: python tools/twin_ab.py [--runs 5] [--out twin_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dmft-ed_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

torch.cuda.init()
import ctypes

from edgpu._lib import check, load
from edgpu.diag import DiagOptions
from edgpu.farm import farm_diag
from edgpu.hamiltonian import Sector
from golden.golden_configs import c4_config

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

cfg = c4_config("random")
out = {"kernel": {}, "farm": {}}
lib = load()
NCALL = 50      # calls per event pair

# ------------------------------------------------------------ 1. the kernels
mk = lambda q, **kw: Sector(cfg, q[0], q[1], stored=False, direct=True, real=True, **kw)   # noqa: E731
with mk((6, 5)) as A, mk((5, 6)) as B, mk((5, 6), options=("twin_gather",)) as Bg:
    dev = torch.device("cuda", 0)
    for name, dt, nbytes in (("real", torch.float64, 16), ("complex", torch.complex128, 32)):
        x = torch.randn(A.dim, dtype=dt, device=dev)
        y = torch.empty_like(x)
        st = torch.cuda.Stream(device=dev)
        P = ctypes.c_void_p
        ms = {"transpose": [], "gather": []}
        with torch.cuda.stream(st):
            for it in range(25):
                for kind, dst in (("transpose", B), ("gather", Bg)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(NCALL):     # back to back: the launch latency overlaps the previous kernel
                        check(lib.ed_sector_twin_vector(A.handle, dst.handle, 1 if dt.is_complex else 0,
                                                        P(x.data_ptr()), P(y.data_ptr()), P(st.cuda_stream)), "twin")
                    e1.record()
                    e1.synchronize()
                    if it >= 5:
                        ms[kind].append(e0.elapsed_time(e1) / NCALL)
        ref = x.cpu().numpy().reshape(int(A.info.dimdw), int(A.info.dimup)).T.reshape(-1)
        assert np.array_equal(A.twin_vector(B, x).cpu().numpy(), ref)
        assert np.array_equal(A.twin_vector(Bg, x).cpu().numpy(), ref)
        for kind, v in ms.items():
            med = statistics.median(v)
            out["kernel"][f"{name}_{kind}"] = {
                "dim": A.dim, "ms_median": med, "ms_min": min(v), "ms_max": max(v), "n": len(v),
                "bytes": nbytes * A.dim, "fraction_of_8TBs": nbytes * A.dim / (med * 1e-3) / 8e12}
            print(name, kind, out["kernel"][f"{name}_{kind}"], flush=True)

# --------------------------------------------------------------- 2. the farm
walls = {False: [], True: []}
nsec = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for tw in (False, True):
        farm_diag(cfg, DiagOptions(ed_twin=tw))          # warm-up
    for _ in range(args.runs):
        for tw in (False, True):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = farm_diag(cfg, DiagOptions(ed_twin=tw))
            torch.cuda.synchronize()
            walls[tw].append(time.perf_counter() - t)
            nsec[tw] = len(r.local)
            e0 = r.states.emin
with open(os.path.join(ROOT, "profiles", "farm_c4_1gpu.json")) as fh:
    base = json.load(fh)["wall_s"]
for tw in (False, True):
    out["farm"]["ed_twin_on" if tw else "ed_twin_off"] = {
        "sectors": nsec[tw], "wall_s_median": statistics.median(walls[tw]), "wall_s": walls[tw]}
out["farm"]["profiles_farm_c4_1gpu_wall_s"] = base
print(out["farm"], flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
