"""Time one kept state of the configs[3] (6,6) sector (dim 853,776, direct build):
nn_moments over the 4 impurity levels, expect with the full local_energy term
list, and the host route (to_host + vectorised numpy walk over Sector.map()).
hipEvent pairs around the calls, 3 warm-ups, (median, minimum) of 20 in ms.
The HBM fraction is 12 (20 complex) bytes per row over the 8 TB/s peak.

    python tools/obs_timing.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dmft-ed_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import obs_truth as ot  # noqa: E402
from edgpu.hamiltonian import Sector  # noqa: E402
from edgpu.observables import energy_terms  # noqa: E402
from edgpu.params import make_config  # noqa: E402

cfg = make_config(Norb=2, Nbath=5, Uloc=(2.0, 2.0, 0.0), Ust=1.0, Jh=0.25, Jx=0.25, Jp=0.25)
cfg.impHloc[0, 0] = np.array([[0.1, 0.2], [0.2, -0.1]])
terms = [t for _, _, t in energy_terms(cfg)]
lv = ot.imp_levels(cfg)
out = {"nterm": len(terms)}


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


with Sector(cfg, 6, 6, stored=False, direct=True, real=True) as S:
    out["dim"] = S.dim
    for cplx in (False, True):
        x = torch.from_numpy(ot.random_state(S.dim, cplx, 1)).cuda()
        torch.cuda.synchronize()
        tag = "complex" if cplx else "real"
        out[f"nn_moments_ms_{tag}"] = timed(lambda: S.nn_moments(x, lv))
        out[f"expect_ms_{tag}"] = timed(lambda: S.expect(x, terms))
        hmap = S.map()

        def host():
            v = x.cpu().numpy()
            ot.numpy_moments(hmap, v, lv)
            return [ot.numpy_expect(hmap, v, t) for t in terms]

        def host_moments():
            v = x.cpu().numpy()
            return ot.numpy_moments(hmap, v, lv)

        out[f"host_moments_ms_{tag}"] = timed(host_moments, n=5, warm=1)
        out[f"host_all_ms_{tag}"] = timed(host, n=3, warm=1)
        # parity of the two routes at this size
        M, norm = S.nn_moments(x, lv)
        Mh, nh = host_moments()
        dv = np.max(np.abs(S.expect(x, terms) - np.array(host())))
        out[f"parity_{tag}"] = [float(np.max(np.abs(M - Mh))), float(abs(norm - nh)), float(dv)]
        vb = 16 if cplx else 8
        out[f"moments_fraction_of_8TBs_{tag}"] = (4 + vb) * S.dim / (out[f"nn_moments_ms_{tag}"][0] * 1e-3) / 8e12

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
