"""HiFi-GAN generator on the HIP path: mel [T', 80] -> waveform [T' * 256] (csrc/hifigan.hip).

The second generator family `parallel-wavegan-decode` (inference_student.sh:20-23) selects by `generator_type`, built from the published
architecture (kan-bayashi/ParallelWaveGAN `HiFiGANGenerator`, v1 / LJSpeech; restated in float64 in tests/hifigan_ref.py -- no upstream source,
checkpoint or vector here: parity unpinned).  State-dict names are that package's, so its checkpoints (`{"model": {"generator": ...}}`, with or
without weight norm) load here; the loader is strict about names and shapes.

Batched: utterances are concatenated row-major (rows = samples at the stage's rate, channels-last); every convolution and the transposed
convolutions see zeros outside their own utterance.  The generator is deterministic: `seed` / `noise` are accepted and unused.  No CPU fallback;
needs the pre-split path (FCL_PRECISION / FCL_PLANES not 0).  `CapacitySynth` is the capacity form (every buffer sized once, the live extent read
from the device): what engine.SpeechRunner captures behind the synthesis pass and what tts.synthesize(vocoder_graph=True) runs; without that flag
tts.synthesize keeps its two-step route for this generator."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .vocoder import Generator, check_capacity, check_run_args, fold_weight_norm

CONFIG = dict(in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
              resblock_kernel_sizes=(3, 7, 11), resblock_dilations=((1, 3, 5), (1, 3, 5), (1, 3, 5)), use_additional_convs=True, bias=True,
              nonlinear_activation="LeakyReLU", nonlinear_activation_params=dict(negative_slope=0.1), use_weight_norm=True)
OUT_SLOPE = 0.01  # the package's output stage is a bare torch.nn.LeakyReLU(): torch's default slope, not negative_slope


def config(cfg=None):
    """CONFIG with overrides, sequences as tuples, checked for what the kernels cover (NotImplementedError names the offending parameter)."""
    c = dict(CONFIG, **(cfg or {}))
    c["upsample_scales"] = tuple(int(s) for s in c["upsample_scales"])
    c["upsample_kernel_sizes"] = tuple(int(s) for s in c["upsample_kernel_sizes"])
    c["resblock_kernel_sizes"] = tuple(int(s) for s in c["resblock_kernel_sizes"])
    c["resblock_dilations"] = tuple(tuple(int(d) for d in ds) for ds in c["resblock_dilations"])
    bad = {}
    if c["nonlinear_activation"] != "LeakyReLU":
        bad["nonlinear_activation"] = c["nonlinear_activation"]
    if not c["use_additional_convs"]:
        bad["use_additional_convs"] = c["use_additional_convs"]
    if not c["bias"]:
        bad["bias"] = c["bias"]
    if len(c["upsample_kernel_sizes"]) != len(c["upsample_scales"]) or any(ku != 2 * s for s, ku in zip(c["upsample_scales"], c["upsample_kernel_sizes"])):
        # ku % s != 0 has no polyphase form; a multiple other than 2 s does not give s x the input length with the package's padding
        bad["upsample_kernel_sizes"] = c["upsample_kernel_sizes"]
    if len(c["resblock_dilations"]) != len(c["resblock_kernel_sizes"]) or any(k not in (3, 5, 7, 11) for k in c["resblock_kernel_sizes"]) or any(
            not 1 <= d <= 5 for ds in c["resblock_dilations"] for d in ds):
        bad["resblock_kernel_sizes / resblock_dilations"] = (c["resblock_kernel_sizes"], c["resblock_dilations"])
    n = len(c["upsample_scales"])
    if c["channels"] % (32 << n) or c["kernel_size"] % 2 == 0 or c["kernel_size"] > 11 or not 1 <= c["out_channels"] <= 4:
        bad["channels / kernel_size / out_channels"] = (c["channels"], c["kernel_size"], c["out_channels"])
    if bad:
        raise NotImplementedError("fcl-taco2_amd: HiFiGANGenerator generator_params %r are not supported on the HIP path" % bad)
    return c


def param_spec(cfg=None):
    """Ordered {state_dict name: shape}, weight norm folded (the generator after remove_weight_norm())."""
    c = config(cfg)
    ch, k, nk = c["channels"], c["kernel_size"], len(c["resblock_kernel_sizes"])
    spec = {"input_conv.weight": (ch, c["in_channels"], k), "input_conv.bias": (ch,)}
    for i, ku in enumerate(c["upsample_kernel_sizes"]):
        ci, co = ch >> i, ch >> (i + 1)
        spec["upsamples.%d.1.weight" % i], spec["upsamples.%d.1.bias" % i] = (ci, co, ku), (co,)  # ConvTranspose1d: dim 0 is the INPUT channel
        for j, kr in enumerate(c["resblock_kernel_sizes"]):
            for d in range(len(c["resblock_dilations"][j])):
                for cv in ("convs1", "convs2"):
                    p = "blocks.%d.%s.%d.1." % (i * nk + j, cv, d)
                    spec[p + "weight"], spec[p + "bias"] = (co, co, kr), (co,)
    cl = ch >> len(c["upsample_scales"])
    spec["output_conv.1.weight"], spec["output_conv.1.bias"] = (c["out_channels"], cl, k), (c["out_channels"],)
    return spec


def tconv_padding(s):
    """(padding, output_padding) of the package's upsampling layers."""
    return s // 2 + s % 2, s % 2


def tconv_rule(x, w, b, s, lens):
    """numpy statement of the transposed-convolution stage (fcl_hfg_tconv_fwd): x [sum(lens), Cin] rows of concatenated utterances, w (Cin, Cout, ku)
    with ku a multiple of s, padding / output_padding as tconv_padding(s).  Output row n = s q + p of an utterance takes, with t = p + padding,
    tap j = 0 .. ku / s - 1: input row q + t // s - j (zero outside the utterance's own rows) times w[:, :, s j + t % s].  -> [sum(lens) * s, Cout]."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ku = w.shape[2]
    if ku % s:
        raise ValueError("tconv_rule: kernel size %d is not a multiple of the stride %d" % (ku, s))
    pad, _ = tconv_padding(s)
    out = np.zeros((x.shape[0] * s, w.shape[1]))
    off = 0
    for n_ in lens:
        for q in range(n_):
            for p in range(s):
                t = p + pad
                acc = np.array(b, dtype=np.float64).copy()
                for j in range(ku // s):
                    i = q + t // s - j
                    if 0 <= i < n_:
                        acc += x[off + i] @ w[:, :, s * j + t % s]
                out[(off + q) * s + p] = acc
        off += n_
    return out


def capacity_maps_rule(utt_frame0, batch, frames_cap, hop, status=0):
    """numpy statement of fcl_hfg_maps_build.  utt_frame0 [batch + 1]: frame starts of the utterance slots ([batch] = total); a slot without
    frames owns no frame.  Frames [live, frames_cap) belong to pseudo-utterance `batch` (utt_off[batch] = live, utt_off[batch + 1] = frames_cap), so
    every index lies inside its buffer.  An incoming status, starts that do not ascend from 0 or more than frames_cap frames: nothing is live and
    the whole capacity is the pseudo-utterance; the last two OR STATUS_VOCODER_CAP into a zero status, an incoming status stays as it is.
    Returns dict(frame_utt [frames_cap], utt_off [batch + 2], live [4] = {frames, samples, 0, utterances with frames}, status, ok)."""
    off = np.asarray(utt_frame0, dtype=np.int64).reshape(-1)[: batch + 1]
    if off.shape[0] != batch + 1:
        raise ValueError("capacity_maps_rule: utt_frame0 must hold batch + 1 = %d frame starts" % (batch + 1))
    fits = off[0] == 0 and bool(np.all(np.diff(off) >= 0)) and off[batch] <= frames_cap
    ok = fits and int(status) == 0
    status_out = int(status) if int(status) != 0 or fits else _lib.STATUS_VOCODER_CAP
    if not ok:
        off = np.zeros(batch + 1, dtype=np.int64)
    live = int(off[batch])
    fu = np.full(frames_cap, batch, dtype=np.int64)
    fu[:live] = np.searchsorted(off[:batch], np.arange(live), side="right") - 1  # (equal starts: the last one, i.e. the slot that has frames)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(frame_utt=i32(fu), utt_off=i32(np.concatenate([off, [frames_cap]])), live=i32([live, live * hop, 0, int((np.diff(off) > 0).sum())]),
                status=status_out, ok=bool(ok))


def _stage_geometry(cfg):
    """[(rows per frame, channels)] of every stage's output"""
    c = config(cfg)
    out, rate = [], 1
    for i, s in enumerate(c["upsample_scales"]):
        rate *= s
        out.append((rate, c["channels"] >> (i + 1)))
    return out


def capacity_nbytes(cfg, batch, frames_cap):
    """Exact byte count of a CapacitySynth's buffers (its `nbytes` adds the allocator's rounding, < 512 B per tensor).  Per capacity frame:
        7 x max_i(rate_i x C_i) x 4      the ONE set of row buffers c, cpl, xb, cs, pa, pb, csp (fp32 or planes: 4 B per row and channel either way)
                                         every stage works in -- a stage's seven are dead once the next stage's transposed convolution has read csp
        + max(rate_i x C_i : C_i wider than 128) x 4     the workspace tp of the one-launch-per-convolution stages (0 without such a stage)
        + channels x 4 + ceil(in_channels / 32) x 128    input_conv's output planes and the mel's planes
        + hop x (4 + 2) x out_channels + 4               wav, pcm and frame_utt
    plus 4 x (batch + 2) + 16 bytes for utt_off and the live record.  v1: 7 x 8192 x 4 = 229 KB of the 241 KB per frame, ~0.94 KB per sample."""
    c = config(cfg)
    geo = _stage_geometry(c)
    hop = geo[-1][0]
    rows = 7 * max(r * ch for r, ch in geo) * 4
    tp = max([r * ch for r, ch in geo if ch not in (32, 64, 128)] + [0]) * 4
    small = c["channels"] * 4 + (c["in_channels"] + 31) // 32 * 128 + hop * 6 * c["out_channels"] + 4
    return int(frames_cap) * (rows + tp + small) + 4 * (int(batch) + 2) + 16


def build_chain(pl, F, fu, uo, melp, cp0, rows_of, y0=None):
    """The descriptors of every launch on F frames, once for the exact form (synthesize_packed) and the capacity form (CapacitySynth).  fu, uo:
    pointers of frame_utt / utt_off; melp, cp0: planes of the mel and of input_conv's output (y0: its fp32 output, where wanted);
    rows_of(rows, channels) -> the row buffers (c, cpl, xb, cs, pa, pb, csp, tp) a stage works in (fp32 c, xb, cs, the others planes; tp only
    read for a width outside 32 / 64 / 128).  The transposed convolution writes c / cpl; the units of a block ping-pong from there through
    xb / pa / pb, the block's last unit adds into cs and the stage's last one writes csp, the planes the next stage (or output_conv) reads.
    Returns (input conv, [(tconv, units)], csp, rows per frame of csp)."""
    ptr = lambda t: None if t is None else t.data_ptr()
    a = _lib.HfgConv()
    a.m, a.cin, a.cout, a.ksize, a.dilation, a.rate, a.slope = F, pl.input["cin"], pl.input["cout"], pl.input["k"], 1, 1, pl.slope
    a.xp, a.wp, a.bias, a.frame_utt, a.utt_off, a.y, a.yp = ptr(melp), ptr(pl.input["wp"]), ptr(pl.input["b"]), fu, uo, ptr(y0), ptr(cp0)
    stages, rate, rows, cp = [], 1, F, cp0
    for si, st in enumerate(pl.stages):
        tc = _lib.HfgTconv()
        tc.m_in, tc.cin, tc.cout, tc.stride, tc.ksize, tc.padding, tc.rate_in, tc.slope = rows, st["cin"], st["cout"], st["s"], st["ku"], \
            tconv_padding(st["s"])[0], rate, pl.slope
        rows, rate, Cc = rows * st["s"], rate * st["s"], st["cout"]
        c, cpl, xb, cs, pa, pb, csp, tp = rows_of(rows, Cc)
        tc.xp, tc.wp, tc.bias, tc.frame_utt, tc.utt_off, tc.y, tc.yp = ptr(cp), ptr(st["wp"]), ptr(st["b"]), fu, uo, ptr(c), ptr(cpl)
        units, nk = [], len(st["blocks"])
        for j, blk in enumerate(st["blocks"]):
            x_in, xp_in, xp_out = c, cpl, pa
            for d, U in enumerate(blk):
                last = d == len(blk) - 1
                u = _lib.HfgUnit()
                u.m, u.c, u.ksize, u.dilation, u.rate, u.first, u.last = rows, Cc, U["k"], U["dilation"], rate, int(j == 0), int(last)
                u.slope, u.cs_scale, u.csp_slope = pl.slope, 1.0 / nk, OUT_SLOPE if si == len(pl.stages) - 1 else pl.slope
                u.xp, u.x, u.w1p, u.b1, u.w2p, u.b2 = ptr(xp_in), ptr(x_in), ptr(U["w1p"]), ptr(U["b1"]), ptr(U["w2p"]), ptr(U["b2"])
                u.frame_utt, u.utt_off = fu, uo
                if last:
                    u.cs, u.csp = ptr(cs), ptr(csp) if j == nk - 1 else None
                else:
                    u.x_out, u.xp_out = ptr(xb), ptr(xp_out)
                u.tp = ptr(tp) if Cc not in (32, 64, 128) else None
                units.append(u)
                x_in, xp_in, xp_out = xb, xp_out, (pb if xp_out is pa else pa)
        stages.append((tc, units))
        cp = csp
    return a, stages, cp, rate


def enqueue_chain(pl, chain, wav, M, oc, s, live=None):
    """Every launch of build_chain's descriptors, then output_conv into wav [M, oc]: the exact entries, or with `live` (the pointer of a capacity
    form's live record) the cap entries, which do no work past the live rows."""
    lib, chk, cap = _lib.load(), _lib.check, () if live is None else (live,)
    conv, tconv, unit, out = (lib.fcl_hfg_conv_fwd, lib.fcl_hfg_tconv_fwd, lib.fcl_hfg_unit_fwd, lib.fcl_hfg_out_fwd) if live is None else (
        lib.fcl_hfg_conv_cap_fwd, lib.fcl_hfg_tconv_cap_fwd, lib.fcl_hfg_unit_cap_fwd, lib.fcl_hfg_out_cap_fwd)
    a, stages, csp, rate = chain
    chk(conv(C.byref(a), *cap, s))
    for tc, units in stages:
        chk(tconv(C.byref(tc), *cap, s))
        for u in units:
            chk(unit(C.byref(u), *cap, s))
    chk(out(csp.data_ptr(), pl.out_w.data_ptr(), pl.out_b.data_ptr(), a.frame_utt, a.utt_off, rate, wav.data_ptr(), M, pl.c_last, oc, pl.cfg["kernel_size"], *cap, s))


class CapacitySynth(object):
    """The generator in CAPACITY form (the surface of vocoder.CapacitySynth): every buffer, descriptor and pointer is fixed at construction for `batch`
    utterance slots and `frames_cap` mel frames; what is live comes from the device (the synthesis pass's frame starts), so `run` derives no host
    value from the data, allocates nothing and is capturable in a hipGraph behind the synthesis pass (engine.SpeechRunner).  The chain is
    fcl_hfg_maps_build -> fcl_pack_planes of the capacity mel -> the conv / tconv / unit / out cap launches -> fcl_pcm16_fwd; the cap launches do no
    work and touch no memory past the live rows, and a live row is computed exactly as `synthesize_packed` computes it on the same packed rows:
    both run build_chain's descriptors through enqueue_chain, here on the one shared set of row buffers.
    Memory: capacity_nbytes (the stages share one set of row buffers); `nbytes` is what this instance holds (its tensors, 512-byte granularity)."""

    def __init__(self, gen, batch, frames_cap, seed=0):
        pl = self.plan = gen.plan
        self.gen, self.B, self.frames_cap, self.seed = gen, int(batch), int(frames_cap), int(seed) & 0xFFFFFFFF
        dev = pl.device
        if pl.out_channels != 1:
            raise _lib.FclError("fcl-taco2_amd: the capacity form of the HiFi-GAN generator writes mono PCM: out_channels = %d is not supported; use "
                                "synthesize_packed for this generator" % pl.out_channels)
        check_capacity(self.B, self.frames_cap, pl.hop)
        F, hop = self.frames_cap, pl.hop
        self.M = F * hop
        geo = _stage_geometry(pl.cfg)
        with torch.cuda.device(dev):
            i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
            self.frame_utt, self.utt_off, self.live = i32(F), i32(self.B + 2), i32(4)
            self.melp = ops.planes_empty(F, pl.A, dev)
            self.cp0 = ops.planes_empty(F, pl.input["cout"], dev)
            width = max(r * ch for r, ch in geo)  # elements per frame of the widest stage
            c, xb, cs = [torch.empty(F * width, device=dev, dtype=torch.float32) for _ in range(3)]
            cpl, pa, pb, csp = [torch.empty(F * width * 2, device=dev, dtype=torch.int16) for _ in range(4)]
            tpw = max([r * ch for r, ch in geo if ch not in (32, 64, 128)] + [0])
            tp = torch.empty(F * tpw * 2, device=dev, dtype=torch.int16) if tpw else None
            self.wav = torch.empty(self.M, device=dev, dtype=torch.float32)
            self.pcm = torch.empty(self.M, device=dev, dtype=torch.int16)
            self._rows = (c, cpl, xb, cs, pa, pb, csp, tp)
            for t_ in (self.melp, self.cp0, cpl, pa, pb, csp) + ((tp,) if tp is not None else ()):
                assert t_.data_ptr() % 128 == 0
            # what this instance holds: its tensors' storages at the caching allocator's 512-byte granularity (a memory_allocated() difference would
            # also count the unsplit remainders of whatever pool blocks the allocator happened to hand out)
            held = (self.frame_utt, self.utt_off, self.live, self.melp, self.cp0, self.wav, self.pcm) + tuple(t_ for t_ in self._rows if t_ is not None)
            self.nbytes = sum((t_.untyped_storage().nbytes() + 511) // 512 * 512 for t_ in held)
            # the descriptors of every launch: every pointer is static, m / m_in is the capacity
            self._chain = build_chain(pl, F, self.frame_utt.data_ptr(), self.utt_off.data_ptr(), self.melp, self.cp0, lambda rows, ch: self._rows)
            # eager warm-up on an empty batch: the library's one-time setup (dynamic-LDS opt-ins) must not happen inside a capture
            self.run(torch.zeros(1, pl.A, device=dev), i32(self.B + 1), i32(1))
            torch.cuda.current_stream(dev).synchronize()

    def run(self, mel_rows_cap, utt_frame0_dev, status, seed_dev=None):
        """Enqueue the whole generator + the PCM conversion on the current stream.  mel_rows_cap: [rows, in_channels] float32 device tensor whose first
        utt_frame0[B] rows are the batch's packed mel frames (later rows may hold anything, NaN included: their planes are never read);
        utt_frame0_dev: int32 [B + 1] on the device; status: the pass's int32 status word (FCL_STATUS_VOCODER_CAP / FCL_STATUS_PCM_NONFINITE are
        OR-ed into it; a word that is already set makes this pass generate nothing); seed_dev: accepted and ignored (the generator draws no noise).
        Results: self.pcm (int16) and self.wav (float32), live samples [0, self.live[1])."""
        pl, lib = self.plan, _lib.load()
        check_run_args(mel_rows_cap, utt_frame0_dev, status, pl.A, self.B)
        s, live, chk = ops._stream(), self.live.data_ptr(), _lib.check
        chk(lib.fcl_hfg_maps_build(utt_frame0_dev.data_ptr(), status.data_ptr(), self.B, self.frames_cap, pl.hop, self.frame_utt.data_ptr(),
                                   self.utt_off.data_ptr(), live, s))
        # (a buffer with fewer rows than the capacity cannot hold more live frames than it has rows: the synthesis pass's own capacity)
        chk(lib.fcl_pack_planes(mel_rows_cap.data_ptr(), mel_rows_cap.stride(0), min(int(mel_rows_cap.shape[0]), self.frames_cap), pl.A, self.melp.data_ptr(), s))
        enqueue_chain(pl, self._chain, self.wav, self.M, 1, s, live)
        chk(lib.fcl_pcm16_fwd(self.wav.data_ptr(), self.pcm.data_ptr(), self.M, live, status.data_ptr(), s))
        return self.pcm


class HiFiGANPlan(object):
    """Device-resident, GEMM-ready weights of one generator: tap-major P32 planes of every convolution, packed once."""

    eager_only = True  # the driver's default route: tts.synthesize takes the two-step route unless vocoder_graph is asked for (CapacitySynth exists)

    def __init__(self, state_dict, device, cfg=None):
        if not ops.planes_enabled():
            raise _lib.FclError("fcl-taco2_amd: the vocoder runs on the pre-split operand kernels only (FCL_PRECISION=0 / FCL_PLANES=0 is set)")
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: HiFiGANPlan needs a GPU device (no CPU fallback)")
        self.cfg = c = config(cfg)
        self.device = dev = torch.device(device)
        if "model" in state_dict and "generator" in state_dict["model"]:  # a parallel_wavegan checkpoint
            state_dict = state_dict["model"]["generator"]
        sd = fold_weight_norm(state_dict)
        check_state_dict(sd, c)
        self.A, self.out_channels = c["in_channels"], c["out_channels"]
        self.hop = int(np.prod(c["upsample_scales"]))
        self.slope = float(c["nonlinear_activation_params"].get("negative_slope", 0.01))
        nk = len(c["resblock_kernel_sizes"])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def taps(w):  # (Cout, Cin, k) -> planes of the tap-major [k * Cout, Cin]
            w = t(w)
            return ops.pack_planes(ops.pack_conv1d_weight(w).reshape(w.shape[2] * w.shape[0], w.shape[1]))

        with torch.cuda.device(dev):
            self.input = dict(wp=taps(sd["input_conv.weight"]), b=t(sd["input_conv.bias"]), k=c["kernel_size"], cin=self.A, cout=c["channels"])
            self.stages = []
            for i, (s, ku) in enumerate(zip(c["upsample_scales"], c["upsample_kernel_sizes"])):
                co = c["channels"] >> (i + 1)
                blocks = []
                for j, kr in enumerate(c["resblock_kernel_sizes"]):
                    units = []
                    for d, dil in enumerate(c["resblock_dilations"][j]):
                        p = "blocks.%d." % (i * nk + j)
                        units.append(dict(k=kr, dilation=dil, w1p=taps(sd[p + "convs1.%d.1.weight" % d]), b1=t(sd[p + "convs1.%d.1.bias" % d]),
                                          w2p=taps(sd[p + "convs2.%d.1.weight" % d]), b2=t(sd[p + "convs2.%d.1.bias" % d])))
                    blocks.append(units)
                self.stages.append(dict(s=s, ku=ku, cin=c["channels"] >> i, cout=co, wp=taps(np.transpose(sd["upsamples.%d.1.weight" % i], (1, 0, 2))),
                                        b=t(sd["upsamples.%d.1.bias" % i]), blocks=blocks))
            self.out_w = ops.pack_conv1d_weight(t(sd["output_conv.1.weight"]))  # [k, out, C_last] fp32
            self.out_b = t(sd["output_conv.1.bias"])
            self.c_last = c["channels"] >> len(c["upsample_scales"])


def check_state_dict(sd, cfg):
    """Every name and shape of param_spec(cfg) must be present, and nothing else: FclError names the first offender."""
    spec = param_spec(cfg)
    for k, shp in spec.items():
        if k not in sd or tuple(np.shape(sd[k])) != tuple(shp):
            raise _lib.FclError("fcl-taco2_amd: HiFi-GAN generator state_dict lacks %s %r (got %r)" % (k, shp, None if k not in sd else tuple(np.shape(sd[k]))))
    extra = sorted(k for k in sd if k not in spec)
    if extra:
        raise _lib.FclError("fcl-taco2_amd: HiFi-GAN generator state_dict holds %s, which the configured geometry does not use" % extra[0])


class HiFiGANGenerator(Generator):
    """The HiFi-GAN generator on a HiFiGANPlan."""

    def capacity_synth(self, batch, frames_cap, seed=0):
        """The capacity form of this generator for `batch` utterance slots and `frames_cap` mel frames (what engine.SpeechRunner captures)."""
        return CapacitySynth(self, batch, frames_cap, seed=seed)

    def synthesize_packed(self, mel_rows, lens, noise=None, seed=0, return_intermediates=False, return_flat=False):
        """Utterances packed row-wise ([sum T', in_channels] device tensor) with their frame counts -> list of [T'_i * hop] float32 device tensors
        ([T'_i * hop, out] for out > 1).  return_intermediates: also a dict with `taps` = [input_conv's output, every stage's output c] (fp32).
        return_flat: also the one buffer the waveforms are slices of."""
        pl, dev = self.plan, self.plan.device
        with torch.cuda.device(dev):
            lens = self._packed_lens(mel_rows, lens)
            F = sum(lens)
            if F * pl.hop >= 2 ** 30:
                raise _lib.FclError("fcl-taco2_amd: more than 2^30 samples in one vocoder batch")
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            frame_utt = torch.from_numpy(np.repeat(np.arange(len(lens)), lens).astype(np.int32)).to(dev)
            utt_off = torch.from_numpy(offs.astype(np.int32)).to(dev)
            f32 = lambda r, c: torch.empty(r, c, device=dev, dtype=torch.float32)
            held = []  # every stage's own row buffers, alive until the launches are enqueued

            def rows_of(rows, ch):  # (c, cpl, xb, cs, pa, pb, csp, tp) at the stage's size
                pe = lambda: ops.planes_empty(rows, ch, dev)
                held.append((f32(rows, ch), pe(), f32(rows, ch), f32(rows, ch), pe(), pe(), pe(), pe() if ch not in (32, 64, 128) else None))
                return held[-1]

            melp = ops.pack_planes(mel_rows.to(torch.float32).contiguous())
            cp0 = ops.planes_empty(F, pl.input["cout"], dev)
            c0 = f32(F, pl.input["cout"]) if return_intermediates else None
            chain = build_chain(pl, F, frame_utt.data_ptr(), utt_off.data_ptr(), melp, cp0, rows_of, c0)
            M, oc = F * pl.hop, pl.out_channels
            flat = torch.empty(M * oc, device=dev, dtype=torch.float32)  # the per-utterance waveforms are slices of this one buffer
            enqueue_chain(pl, chain, flat, M, oc, ops._stream())
            outs = [flat[int(offs[i]) * pl.hop * oc : int(offs[i + 1]) * pl.hop * oc] for i in range(len(lens))]
            if oc > 1:
                outs = [o.reshape(-1, oc) for o in outs]
            return self._results(outs, dict(taps=[c0] + [b[3] for b in held], lens=lens), flat, return_intermediates, return_flat)
