"""Cost of the radiation launches per step at the shape of benchmark config C2 (1024^2 cells, 64 per cell, thermal: no
event fires, so this times the event kernel and the two host reads -- the emit kernel and the store growth are NOT in it).
Three engines side by side -- the one-call lpa_step route, the per-stage calls, the per-stage calls with radiation -- timed
in alternating rounds of --steps steps (host clock around a device synchronise); prints the per-round ms per step."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from lambdapic_amd import constants  # noqa: E402
from lambdapic_amd.engine import PicEngine2D  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--ppc", type=int, default=64)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=4)
args = ap.parse_args()
NX = NY = args.n
DX = 4e-8
DT = 0.95 / (constants.C_LIGHT * np.sqrt(2) / DX)


def make(mode):
    eng = PicEngine2D(NX, NY, DX, DX, sort_interval=20)
    n = NX * NY * args.ppc
    g = torch.Generator(device="cuda").manual_seed(1)
    for q, m, k in ((-constants.E_CHARGE, constants.M_E, n), (0.0, 0.0, 0)):
        s = eng.species[eng.add_species(q, m, capacity=max(k, 1024))]
        if k:
            d = s.cset.data
            for r, ncell in ((0, NX), (1, NY)):
                d[r, :k] = (torch.rand(k, generator=g, device="cuda", dtype=torch.float64) * ncell - 0.5) * DX
            d[2:5, :k] = torch.randn((3, k), generator=g, device="cuda", dtype=torch.float64) * 0.044
            d[5, :k] = 1 / torch.sqrt(1 + (d[2:5, :k] ** 2).sum(0))
            d[6, :k] = 1e27 * DX * DX / args.ppc
            s.cset.id[:k] = torch.arange(k, device="cuda")
        s.n = k
    eng.fused_step = mode == "one_call"
    if mode == "radiation":
        eng.add_radiation(0, 1, seed=1)
    return eng


engines = {m: make(m) for m in ("one_call", "stages", "radiation")}
out = {m: [] for m in engines}
for rnd in range(args.rounds + 1):          # (round 0: warm-up, not recorded)
    for m, eng in engines.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps if rnd else 20):
            eng.step(DT)
        torch.cuda.synchronize()
        if rnd:
            out[m].append(round((time.perf_counter() - t0) / args.steps * 1e3, 4))
print(json.dumps({"ms_per_step_per_round": out}))
