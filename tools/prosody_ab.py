"""Developer tool: cost of prosody control on the captured pass.  Same-box A/B of ms per batch-32 engine.BatchRunner pass with predicted durations
(FCL-taco2-S, synthetic weights with a usable duration head): controls=False against controls=True with a non-identity control (duration scale 1,
so both passes decode the same frames), interleaved A B A B ... on one stream; prints one JSON line."""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import fcl_taco2_amd  # noqa: F401
from fcl_taco2_amd import engine, hparams as HP, ops, prosody as P, synthetic as SYN
from fcl_taco2_amd.plan import SynthesisPlan

dev = "cuda:0"
torch.set_num_threads(4)
B, T_CAP, ROUNDS, REPS = 32, 100, 7, 20
hp = HP.student_hparams(dropout_rate=0.0)
plan = SynthesisPlan(SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(hp))), hp, dev)
xs, _ = SYN.batch_c2(hp.idim, batch=B, t_hi=T_CAP, seed=1234)
ctl = P.ProsodyControl(pitch_shift=0.25, energy_scale=1.1)
_, _, inter = engine.run(plan, engine.prepare(plan, xs), ops.DROP_NONE, return_intermediates=True)
caps = engine.Caps.for_batches([inter["maps"]], slack_steps=2)
stream = torch.cuda.Stream(device=dev)
runners = {"uncontrolled": engine.BatchRunner(plan, B, T_CAP, caps, forced=False, stream=stream, seed=1),
           "controlled": engine.BatchRunner(plan, B, T_CAP, caps, forced=False, stream=stream, seed=1, controls=True)}
runners["uncontrolled"].load(xs)
runners["controlled"].load(xs, prosody=ctl)
frames = {k: r.frames() if r.replay() is not None else None for k, r in runners.items()}
assert frames["controlled"] == frames["uncontrolled"], "a duration scale of 1 must decode the same frames"
ms = {k: [] for k in runners}
for _ in range(ROUNDS):
    for k, r in runners.items():
        stream.synchronize()
        t = time.perf_counter()
        for _ in range(REPS):
            r.replay()
        stream.synchronize()
        ms[k].append(1e3 * (time.perf_counter() - t) / REPS)
med = {k: float(np.median(v)) for k, v in ms.items()}
print(json.dumps({"batch": B, "t_cap": T_CAP, "frames": int(sum(frames["controlled"])), "ms_per_pass_median": med,
                  "controlled_over_uncontrolled": med["controlled"] / med["uncontrolled"], "ms_per_pass_all": ms}))
