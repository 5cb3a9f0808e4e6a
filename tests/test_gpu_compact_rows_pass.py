"""-m gpu: a capacity pass on COMPACT phoneme rows (engine.Caps.rows, the default) against the same pass on the padded [batch, t_cap] rows
(FCL_COMPACT_ROWS=0, read when a BatchRunner is built), student hparams, prenet dropout on with equal seeds: two BatchRunners on the same batches must
give the same valid mel rows bit for bit and the same frame counts -- forced and predicted durations, a smaller batch then a larger one through one
graph, prosody controls -- and the library's launch record must show the front-end and hoist launches sized by the row capacity."""
import numpy as np
import pytest
import torch

from helpers import np_state_dict
from fcl_taco2_amd import hparams as HP, synthetic as SYN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def plans():
    from fcl_taco2_amd.plan import SynthesisPlan

    hp = HP.student_hparams()
    sd = np_state_dict(hp)
    return hp, SynthesisPlan(sd, hp, DEV), SynthesisPlan(SYN.positive_duration_head(sd), hp, DEV)


def batch(hp, lens, seed):
    g = np.random.RandomState(seed)
    return [g.randint(1, hp.idim, size=n).astype(np.int64) for n in lens], [g.randint(1, 7, size=n).astype(np.int64) for n in lens]


def pair(monkeypatch, plan, B, T, caps, **kw):
    """(compact runner, padded runner): the same capacities, seeds and graph contents but for the row universe."""
    from fcl_taco2_amd import engine

    monkeypatch.setenv("FCL_COMPACT_ROWS", "1")
    on = engine.BatchRunner(plan, B, T, caps, seed=5, **kw)
    monkeypatch.setenv("FCL_COMPACT_ROWS", "0")
    off = engine.BatchRunner(plan, B, T, caps, seed=5, **kw)
    assert off.R is None and off.prep.ids.numel() == B * T
    return on, off


def same_pass(on, off, load):
    load(on)
    load(off)
    mel_on, mel_off = on.replay(), off.replay()
    f_on, f_off = on.frames(), off.frames()
    assert f_on == f_off and min(f_on) > 0
    n = sum(f_on)
    assert torch.equal(mel_on[:n], mel_off[:n])
    return f_on


def forced_caps(engine, sets, T):
    maps = [engine.build_row_maps([len(x) for x in xs], ds, T) for xs, ds in sets]
    return engine.Caps.for_batches(maps, slack_steps=1), maps


def test_forced_durations_a_smaller_batch_then_a_larger_one_through_one_graph(plans, monkeypatch):
    from fcl_taco2_amd import engine

    hp, plan, _ = plans
    B, T = 4, 12  # a capacity of four utterances, so that three full ones (36 rows) stay below the padded 48
    sets = [batch(hp, (1, 12, 5), 1), batch(hp, (12, 12, 12), 2)]
    caps, maps = forced_caps(engine, sets, T)
    assert caps.rows == 36
    on, off = pair(monkeypatch, plan, B, T, caps, forced=True)
    assert on.R == 36 and on.prep.ids.numel() == 36 and on.prep.n_rows == 36
    for i in (0, 1, 0):
        xs, ds = sets[i]
        assert same_pass(on, off, lambda r: r.load(xs, ds)) == list(maps[i].utt_frames)
    with pytest.raises(ValueError, match="row capacity"):
        on.load(*batch(hp, (12, 12, 12, 1), 3))
    assert same_pass(on, off, lambda r: None) == list(maps[0].utt_frames)  # the refused load left the previous block in place


def test_a_row_capacity_that_is_the_padded_universe_keeps_the_padded_layout(plans):
    from fcl_taco2_amd import engine

    hp, plan, _ = plans
    caps, _ = forced_caps(engine, [batch(hp, (12, 12, 12), 2)], 12)
    assert caps.rows == 36 and engine.BatchRunner(plan, 3, 12, caps, forced=True).R is None  # B = 3, T = 12: nothing to save


def test_forced_durations_one_tile_with_rows_of_three_utterances(plans, monkeypatch):
    from fcl_taco2_amd import engine

    hp, plan, _ = plans
    sets = [batch(hp, (61, 5, 70), 4)]
    caps, maps = forced_caps(engine, sets, 70)
    on, off = pair(monkeypatch, plan, 3, 70, caps, forced=True)
    assert on.R == 136
    xs, ds = sets[0]
    assert same_pass(on, off, lambda r: r.load(xs, ds)) == list(maps[0].utt_frames)


@pytest.mark.parametrize("controls", [False, True], ids=["plain", "prosody"])
def test_predicted_durations_with_zero_duration_rows_behind_the_total(plans, monkeypatch, controls):
    """The graph predicts the durations; the rows between a batch's total and the capacity are padding rows of duration 0."""
    from fcl_taco2_amd import engine
    from fcl_taco2_amd.prosody import ProsodyControl

    hp, _, plan = plans
    B, T, R = 4, 12, 40
    caps = engine.Caps(64, B * T * 32, np.full(64, B * T, dtype=np.int32), rows=R)
    on, off = pair(monkeypatch, plan, B, T, caps, forced=False, controls=controls)
    assert on.R == R and (on.caps.bounds == R).all()
    g = np.random.RandomState(8)
    for lens, seed in (((1, 12, 5), 1), ((12, 12, 12), 2), ((7, 3), 6)):
        xs, _ = batch(hp, lens, seed)
        ctl = [ProsodyControl(duration_scale=1.5, pitch_scale=g.uniform(0.7, 1.4, n), energy_shift=g.uniform(-0.5, 0.5, n)) for n in lens] if controls else None
        same_pass(on, off, lambda r: r.load(xs, prosody=ctl))


def test_the_launch_record_reports_the_row_capacity(plans, monkeypatch):
    """One eager pass over each runner's loaded block under the launch record.  Off: the front end runs over B * T rows; on: over caps.rows.  The
    entries are sums over the launches of a name, so a name's rows may only drop by a multiple of the difference; the launches that scale with the
    universe are the two encoder convolutions, the two input projections, the two predictor convolutions and the two hoist GEMMs."""
    from fcl_taco2_amd import _lib, engine, ops

    hp, plan, _ = plans
    B, T = 3, 70
    sets = [batch(hp, (61, 5, 70), 4)]
    caps, _ = forced_caps(engine, sets, T)
    on, off = pair(monkeypatch, plan, B, T, caps, forced=True)
    R, rec = on.R, {}
    for name, r in (("on", on), ("off", off)):
        r.load(*sets[0])
        with torch.cuda.stream(r.stream):
            r._feed(False)
            _lib.prof_enable(True)
            engine.run(plan, r.prep, seed=5, seed_dev=r.seed_word, caps=r.caps, status=r.status)
        r.stream.synchronize()
        rec[name] = _lib.prof_collect()
        _lib.prof_enable(False)
        assert int(r.status.item()) == 0
    assert any(k.endswith("/rows") for k in rec["on"]) and not any(k.endswith("/rows") for k in rec["off"])

    def families(d):
        """{kernel family: [launches, rows]}: a GEMM's tile shape (its template arguments) may follow the row count, its family does not."""
        out = {}
        for k, v in d.items():
            f = out.setdefault(k.replace("/rows", "").split("<")[0], [0, 0])
            f[0] += v["launches"]
            f[1] += int(v["rows"])
        return out

    f_on, f_off = families(rec["on"]), families(rec["off"])
    print("on: %r\noff: %r" % (f_on, f_off))
    assert {k: v[0] for k, v in f_on.items()} == {k: v[0] for k, v in f_off.items()}
    for k in ("embed_conv_table_kernel", "variance_embed_rows_kernel", "bilstm_ksplit_kernel+maps"):
        assert f_off[k] == [1, B * T] and f_on[k] == [1, R], (k, f_off[k], f_on[k])
    shrunk = {}
    for k, (launches, rows) in f_on.items():
        diff = f_off[k][1] - rows
        assert diff >= 0 and diff % (B * T - R) == 0 and diff // (B * T - R) <= launches, (k, diff)
        shrunk[k] = diff // (B * T - R)
    named = ("embed_conv_table_kernel", "variance_embed_rows_kernel", "bilstm_ksplit_kernel+maps")
    assert sum(v for k, v in shrunk.items() if k not in named) >= 8, shrunk  # the GEMM and stencil launches listed above
