"""-m gpu: which front-end kernels a synthesis pass launches, from the library's launch record.  By default the embedding gather is gone and the
first encoder convolution is the table kernel (fcl_embed_conv_table_fwd); FCL_EMBED_CONV_TABLE=0 (read when a plan is built: a child process)
brings back the earlier launches.  The table form moves the mel by rounding noise only, with host-built and with device-built row maps alike."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import np_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = {"embed_conv_table_kernel"}
OLD = {"gather_rows_kernel<long>"}

CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, %(tests)r)
import test_gpu_frontend_switches as T
print("NAMES " + json.dumps(T.record()[0]))
"""


def record():
    """One eager pass with forced durations under the launch record: (sorted kernel names, mel, plan, batch)."""
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, engine, hparams as HP, synthetic as SYN
    from fcl_taco2_amd.plan import SynthesisPlan

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = SynthesisPlan(np_state_dict(hp), hp, DEV)
    xs, ds = SYN.batch_c2(hp.idim, batch=3, t_lo=5, t_hi=9, seed=5)
    _lib.prof_enable(True)
    mel = torch.cat(engine.synthesize(plan, xs, ds))
    torch.cuda.synchronize()
    names = sorted(_lib.prof_collect())
    _lib.prof_enable(False)
    return names, mel, plan, (xs, ds)


def test_default_launches_the_table_kernel_and_a_plan_without_tables_agrees():
    from fcl_taco2_amd import engine

    if os.environ.get("FCL_EMBED_CONV_TABLE", "1") in ("", "0"):
        pytest.skip("the front-end switch is off in this process")
    names, mel, plan, (xs, ds) = record()
    assert NEW <= set(names) and not (OLD & set(names)), names
    maps = engine.build_row_maps([len(x) for x in xs], ds, max(len(x) for x in xs))
    mel_dev = torch.cat(engine.synthesize(plan, xs, ds, caps=engine.Caps.from_maps(maps)))
    assert torch.equal(mel_dev, mel)
    # the same plan without its tables launches the gather and the stencil: the first convolution's outputs differ by its bf16x3 rounding
    # (< 3e-5, tests/test_gpu_embed_conv_table.py); on the mel that stays below the 2e-5 the suite allows between two tilings of one pass
    plan.embed_conv_tables = None
    old = torch.cat(engine.synthesize(plan, xs, ds))
    assert old.shape == mel.shape and float((old - mel).abs().max()) < 2e-5


def test_switch_off_gives_the_earlier_launches_in_a_child_process():
    env = dict(os.environ, FCL_EMBED_CONV_TABLE="0")
    r = subprocess.run([sys.executable, "-c", CHILD % dict(tests=os.path.join(ROOT, "tests"))], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = set(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("NAMES ")][-1][6:]))
    assert OLD <= names and not (NEW & names), sorted(names)
