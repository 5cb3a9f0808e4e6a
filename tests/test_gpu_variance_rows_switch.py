"""-m gpu: what a plain planes-mode synthesis pass launches for the variance embedding, from the library's launch record.  By default the embedding is
written straight as the decoder's sorted rows (variance_embed_rows_kernel: no embed-all-rows launch, no gather of its result).  FCL_VAR_EMBED_ROWS=0
(read once per process: a child process) brings back the two earlier launches: no such kernel in the record, every other recorded kernel launched as
often as before -- and the same mel, bit for bit."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from helpers import np_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = "variance_embed_rows_kernel"

CHILD = r"""
import json, sys
sys.path.insert(0, %(tests)r)
import test_gpu_variance_rows_switch as T
print("RECORD " + json.dumps(T.record()))
"""


def record():
    """One eager pass with forced durations under the launch record: {"launches": {kernel name: launches}, "mel": SHA-256 of the mel}."""
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, engine, hparams as HP, synthetic as SYN
    from fcl_taco2_amd.plan import SynthesisPlan

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = SynthesisPlan(np_state_dict(hp), hp, DEV)
    xs, ds = SYN.batch_c2(hp.idim, batch=3, t_lo=5, t_hi=9, seed=5)
    _lib.prof_enable(True)
    mel = torch.cat(engine.synthesize(plan, xs, ds))
    torch.cuda.synchronize()
    launches = {k: v["launches"] for k, v in _lib.prof_collect().items()}
    _lib.prof_enable(False)
    return dict(launches=launches, mel=hashlib.sha256(mel.cpu().numpy().tobytes()).hexdigest())


def test_default_pass_against_a_child_with_the_switch_off():
    if os.environ.get("FCL_VAR_EMBED_ROWS", "1") in ("", "0"):
        pytest.skip("the switch is off in this process")
    new = record()
    assert new["launches"].get(NEW) == 1, sorted(new["launches"])
    env = dict(os.environ, FCL_VAR_EMBED_ROWS="0")
    r = subprocess.run([sys.executable, "-c", CHILD % dict(tests=os.path.join(ROOT, "tests"))], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    old = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:])
    assert NEW not in old["launches"], sorted(old["launches"])
    rest = {k: v for k, v in new["launches"].items() if k != NEW}
    assert rest == old["launches"]
    assert new["mel"] == old["mel"]  # the fused launch is bit-identical to the two it replaces


def test_a_pass_that_returns_intermediates_keeps_the_two_launches():
    """return_intermediates needs the fp32 sum's inputs (p_embs / e_embs): that pass is not routed to the new entry."""
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, engine, hparams as HP, synthetic as SYN
    from fcl_taco2_amd.plan import SynthesisPlan

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = SynthesisPlan(np_state_dict(hp), hp, DEV)
    xs, ds = SYN.batch_c2(hp.idim, batch=3, t_lo=5, t_hi=9, seed=5)
    ref = torch.cat(engine.synthesize(plan, xs, ds))
    _lib.prof_enable(True)
    mels, inter = engine.synthesize(plan, xs, ds, return_intermediates=True)
    torch.cuda.synchronize()
    names = set(_lib.prof_collect())
    _lib.prof_enable(False)
    assert NEW not in names and inter["p_embs"] is not None and inter["e_embs"] is not None
    assert torch.equal(torch.cat(mels), ref)
