"""Parallel WaveGAN generator on the HIP path (BASELINE configs[4]): mel [T', 80] -> waveform [T' * 256].

The reference hands its mels to the external `parallel-wavegan-decode --checkpoint vocoder/PWG/PWG.pkl` (inference_student.sh:20-23); this module
is that stage, built from the published architecture (kan-bayashi/ParallelWaveGAN `ParallelWaveGANGenerator`, v1 / LJSpeech; restated in
oracle/pwg_oracle.py — no source or vectors in the reference: parity unpinned).  State-dict names and the `inference(c, x=None)` call are that
package's, so its checkpoints (`{"model": {"generator": ...}}`, with or without weight norm) load here.

Batched: utterances are concatenated sample-major; every convolution of the 30-layer residual stack is a K-term of the pre-split-operand GEMM
(csrc/pwg.hip).  No CPU fallback; needs the pre-split path (FCL_PRECISION / FCL_PLANES not 0)."""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, ops

CONFIG = dict(layers=30, stacks=3, residual_channels=64, gate_channels=128, skip_channels=64, aux_channels=80, aux_context_window=2,
              kernel_size=3, upsample_scales=(4, 4, 4, 4))


def param_spec(cfg=None):
    """Ordered {state_dict name: shape}, weight norm folded (the generator after remove_weight_norm())."""
    cfg = dict(CONFIG, **(cfg or {}))
    R, G, S, A, k = cfg["residual_channels"], cfg["gate_channels"], cfg["skip_channels"], cfg["aux_channels"], cfg["kernel_size"]
    spec = {"first_conv.weight": (R, 1, 1), "first_conv.bias": (R,), "upsample_net.conv_in.weight": (A, A, 2 * cfg["aux_context_window"] + 1)}
    for i, s in enumerate(cfg["upsample_scales"]):
        spec["upsample_net.upsample.up_layers.%d.weight" % (2 * i + 1)] = (1, 1, 1, 2 * s + 1)
    for l in range(cfg["layers"]):
        p = "conv_layers.%d." % l
        spec[p + "conv.weight"], spec[p + "conv.bias"] = (G, R, k), (G,)
        spec[p + "conv1x1_aux.weight"] = (G, A, 1)
        spec[p + "conv1x1_out.weight"], spec[p + "conv1x1_out.bias"] = (R, G // 2, 1), (R,)
        spec[p + "conv1x1_skip.weight"], spec[p + "conv1x1_skip.bias"] = (S, G // 2, 1), (S,)
    spec["last_conv_layers.1.weight"], spec["last_conv_layers.1.bias"] = (S, S, 1), (S,)
    spec["last_conv_layers.3.weight"], spec["last_conv_layers.3.bias"] = (1, S, 1), (1,)
    return spec


def fold_weight_norm(sd):
    """weight_g / weight_v pairs (torch.nn.utils.weight_norm, norm over every dim but 0) -> plain weights; other entries pass through."""
    out = {}
    for k, v in sd.items():
        v = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v)
        if k.endswith("weight_g"):
            base = k[: -len("_g")]
            vv = sd[base + "_v"]
            vv = np.asarray(vv.detach().cpu().numpy() if torch.is_tensor(vv) else vv, dtype=np.float64)
            norm = np.sqrt((vv.reshape(vv.shape[0], -1) ** 2).sum(axis=1)).reshape([-1] + [1] * (vv.ndim - 1))
            out[base] = (v.astype(np.float64) * vv / norm).astype(np.float32)
        elif not k.endswith("weight_v"):
            out[k] = v
    return out


def unpack_planes(p, cols, chunk_major=False):
    """fp32 value hi + lo of a P32 plane buffer [rows, ceil(cols/32) * 64], row-major or chunk-major ([chunk][row] lines) (tests / debugging: plain
    tensor reshuffling, no arithmetic kernel of ours)."""
    rows = p.shape[0]
    v = (p.reshape(-1, rows, 2, 32).permute(1, 0, 2, 3) if chunk_major else p.reshape(rows, -1, 2, 32)).to(torch.int32)
    f = lambda t: (t << 16).view(torch.float32)
    return (f(v[:, :, 0]) + f(v[:, :, 1])).reshape(rows, -1)[:, :cols].contiguous()


class PWGPlan(object):
    """Device-resident, GEMM-ready weights of one generator: packed taps and their P32 planes, stacked out / skip projections."""

    def __init__(self, state_dict, device, cfg=None):
        if not ops.planes_enabled():
            raise _lib.FclError("fcl-taco2_amd: the vocoder runs on the pre-split operand kernels only (FCL_PRECISION=0 / FCL_PLANES=0 is set)")
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: PWGPlan needs a GPU device (no CPU fallback)")
        self.cfg = cfg = dict(CONFIG, **(cfg or {}))
        self.device = dev = torch.device(device)
        if "model" in state_dict and "generator" in state_dict["model"]:  # a parallel_wavegan checkpoint
            state_dict = state_dict["model"]["generator"]
        sd = fold_weight_norm(state_dict)
        for k, shp in param_spec(cfg).items():
            if k not in sd or tuple(np.shape(sd[k])) != tuple(shp):
                raise _lib.FclError("fcl-taco2_amd: generator state_dict lacks %s %r (got %r)" % (k, shp, None if k not in sd else np.shape(sd[k])))
        self.R, self.A, self.S, self.k = cfg["residual_channels"], cfg["aux_channels"], cfg["skip_channels"], cfg["kernel_size"]
        if cfg["gate_channels"] != 2 * self.R or self.S != self.R or self.R % 32:
            raise _lib.FclError("fcl-taco2_amd: the vocoder kernels need gate = 2 x residual = 2 x skip channels, a multiple of 32")
        self.hop = int(np.prod(cfg["upsample_scales"]))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        with torch.cuda.device(dev):
            self.first_w, self.first_b = t(sd["first_conv.weight"].reshape(-1)), t(sd["first_conv.bias"])
            self.conv_in = ops.pack_conv1d_weight(t(sd["upsample_net.conv_in.weight"]))  # [k, A, A]
            self.up_w = [t(sd["upsample_net.upsample.up_layers.%d.weight" % (2 * i + 1)].reshape(-1)) for i in range(len(cfg["upsample_scales"]))]
            self.layers = []
            for l in range(cfg["layers"]):
                p = "conv_layers.%d." % l
                wp = ops.pack_conv1d_weight(t(sd[p + "conv.weight"]))  # [k, 2R, R]
                w_os = np.concatenate([sd[p + "conv1x1_out.weight"].reshape(self.R, self.R), sd[p + "conv1x1_skip.weight"].reshape(self.S, self.R)])
                self.layers.append(dict(
                    dilation=2 ** (l % (cfg["layers"] // cfg["stacks"])),
                    w_conv_p=ops.pack_planes(wp.reshape(self.k * 2 * self.R, self.R)), b_conv=t(sd[p + "conv.bias"]),
                    w_aux_p=ops.pack_planes(t(sd[p + "conv1x1_aux.weight"].reshape(2 * self.R, self.A))),
                    w_os_p=ops.pack_planes(t(w_os)), b_os=t(np.concatenate([sd[p + "conv1x1_out.bias"], sd[p + "conv1x1_skip.bias"]]))))
            # every block's conv1x1_aux stacked [layers * 2R, A]: the frame-rate form of the auxiliary term projects the features once for all blocks
            self.w_aux_all_p = ops.pack_planes(t(np.concatenate([sd["conv_layers.%d.conv1x1_aux.weight" % l].reshape(2 * self.R, self.A)
                                                                 for l in range(cfg["layers"])])))
            self.last_w1p = ops.pack_planes(t(sd["last_conv_layers.1.weight"].reshape(self.S, self.S)))
            self.last_b1 = t(sd["last_conv_layers.1.bias"])
            self.last_w2 = t(sd["last_conv_layers.3.weight"].reshape(-1))
            self.last_b2 = float(np.asarray(sd["last_conv_layers.3.bias"]).reshape(-1)[0])


def fused_block(plan):
    """One launch per residual block: the published v1 geometry (64 residual channels, kernel 3, <= 96 auxiliary channels); FCL_PWG_FUSED=0 opts out."""
    return plan.R == 64 and plan.k == 3 and plan.A <= 96 and os.environ.get("FCL_PWG_FUSED", "1") != "0"


def aux_frame_rate(plan):
    """The one-launch block with the auxiliary term evaluated at frame rate (default; FCL_PWG_AUX_FRAME_RATE=0 = planes of the upsampled features)."""
    return fused_block(plan) and plan.hop % 128 == 0 and os.environ.get("FCL_PWG_AUX_FRAME_RATE", "1") != "0"


def pcm16_rule(x):
    """float waveform -> little-endian int16, the rule of vocoder_decode.write_wav and of fcl_pcm16_fwd: clip(rint(double(x) * 32767), -32768, 32767),
    ties to even; a non-finite sample becomes 0 (the device kernel also raises FCL_STATUS_PCM_NONFINITE for it)."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    return np.where(fin, np.clip(np.rint(np.where(fin, x, 0.0) * 32767.0), -32768, 32767), 0.0).astype("<i2")


def pcm16(wav):
    """float32 device waveform (any shape, contiguous) -> int16 host array by fcl_pcm16_fwd (the rule of pcm16_rule, on the device: half the
    device-to-host bytes).  Synchronising; raises FclError when the waveform holds a non-finite sample."""
    wav = wav.reshape(-1)
    n = wav.numel()
    with torch.cuda.device(wav.device):
        pcm = torch.empty(n, dtype=torch.int16, device=wav.device)
        st = torch.zeros(1, dtype=torch.int32, device=wav.device)
        _lib.check(_lib.load().fcl_pcm16_fwd(wav.data_ptr(), pcm.data_ptr(), n, None, st.data_ptr(), ops._stream()))
        host = pcm.cpu().numpy()
        bits = int(st.item()) & 0xFFFFFFFF
    if bits:
        raise _lib.FclError("fcl-taco2_amd: device status 0x%x: %s" % (bits, ops.status_message(bits)))
    return host


def capacity_sizes(batch, frames_cap, ctx, hop):
    """Element counts of the capacity maps (fcl_pwg_maps_build): padded frame rows, samples."""
    return int(frames_cap) + 2 * int(ctx) * (int(batch) + 1), int(frames_cap) * int(hop)


def capacity_maps_rule(utt_frame0, frames_cap, ctx, hop, status=0):
    """numpy statement of fcl_pwg_maps_build: the vocoder's index maps of a batch, to capacity.  utt_frame0 [B + 1]: frame starts of the B utterance
    slots ([B] = total); an utterance without frames contributes nothing.  On the live extent the maps are those of `_maps([frames of the
    utterances that have frames])`, with frame_utt / utt_off numbered by SLOT; frames [live, frames_cap) are one pseudo-utterance (index B) that owns
    the rest of every buffer.  Returns a dict of int32 arrays + live = [frames, samples, padded rows, utterances with frames] + ok (False: incoming
    status, frame starts that do not ascend from 0, or more frames than frames_cap -> nothing is live)."""
    off = np.asarray(utt_frame0, dtype=np.int64).reshape(-1)
    B = off.shape[0] - 1
    ok = int(status) == 0 and off[0] == 0 and bool(np.all(np.diff(off) >= 0)) and off[B] <= frames_cap
    if not ok:
        off = np.zeros(B + 1, dtype=np.int64)
    n = np.diff(off)
    has = n > 0
    pb = np.concatenate([[0], np.cumsum(np.where(has, n + 2 * ctx, 0))])  # first padded row of each slot; [B] = live padded rows
    live, live_pad = int(off[B]), int(pb[B])
    pad_cap, m_cap = capacity_sizes(B, frames_cap, ctx, hop)
    f = np.arange(frames_cap, dtype=np.int64)
    fu = np.full(frames_cap, B, dtype=np.int64)
    fu[:live] = np.searchsorted(off, f[:live], side="right") - 1  # (equal starts: the last one, i.e. the slot that has frames)
    keep = live_pad + ctx + (f - live)
    keep[:live] = pb[fu[:live]] + ctx + (f[:live] - off[fu[:live]])
    j = np.arange(pad_cap, dtype=np.int64)
    pad_idx, lo, hi = np.zeros(pad_cap, dtype=np.int64), np.full(pad_cap, live_pad, dtype=np.int64), np.full(pad_cap, pad_cap, dtype=np.int64)
    pu = np.minimum(np.searchsorted(pb, j[:live_pad], side="right") - 1, max(B - 1, 0))
    pad_idx[:live_pad] = off[pu] + np.clip(j[:live_pad] - pb[pu] - ctx, 0, n[pu] - 1)
    lo[:live_pad] = pb[pu]
    hi[:live_pad] = pb[pu] + n[pu] + 2 * ctx
    su = np.repeat(fu, hop)
    offx = np.concatenate([off, [frames_cap]])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(pad_idx=i32(pad_idx), lo=i32(lo), hi=i32(hi), keep=i32(keep), frame_utt=i32(fu), utt_off=i32(offx), seg_lo=i32(offx[su] * hop),
                seg_hi=i32(offx[su + 1] * hop), live=i32([live, live * hop, live_pad, int(has.sum())]), ok=ok)


def check_capacity(batch, frames_cap, hop):
    """The range of a capacity form's `batch` utterance slots and `frames_cap` mel frames"""
    if batch < 1 or batch > 1024 or frames_cap < 1 or frames_cap * hop >= 2 ** 31 - 1:
        raise _lib.FclError("fcl-taco2_amd: capacity vocoder: 1..1024 utterances and fewer than 2^31 / hop frames expected (got %d, %d)" % (batch, frames_cap))


def check_run_args(mel_rows_cap, utt_frame0_dev, status, aux, batch):
    """What a capacity form's `run` refuses"""
    if mel_rows_cap.dim() != 2 or mel_rows_cap.shape[1] != aux or mel_rows_cap.dtype != torch.float32 or not mel_rows_cap.is_contiguous():
        raise _lib.FclError("fcl-taco2_amd: capacity vocoder: expected contiguous float32 [rows, %d] mel rows, got %r" % (aux, tuple(mel_rows_cap.shape)))
    if utt_frame0_dev.dtype != torch.int32 or utt_frame0_dev.numel() < batch + 1 or status.dtype != torch.int32:
        raise _lib.FclError("fcl-taco2_amd: capacity vocoder: utt_frame0 must hold %d int32 frame starts and status be an int32 word" % (batch + 1))


# ---- the launch chain, once for the exact form (synthesize_packed: buffers of the batch's size, allocated per call) and the capacity form
# (CapacitySynth: buffers of the capacity, allocated once).  Nothing below allocates or reads a device value back.
def cascade(pl, c, frame_utt, utt_off, frames, chunk_major, outs):
    """The 4 x (stretch + smoothing) stages on c [frames, C] (C % 4 == 0) into `outs`, one buffer per stage: fp32 [frames * rate, C], or int16 for
    the planes of that stage's result.  Returns the last one."""
    lib, C_, rate = _lib.load(), c.shape[1], 1
    for s, w, out in zip(pl.cfg["upsample_scales"], pl.up_w, outs):
        as_planes = out.dtype == torch.int16
        _lib.check(lib.fcl_pwg_upsample_stage(c.data_ptr(), frame_utt.data_ptr(), utt_off.data_ptr(), frames, rate, s, w.data_ptr(),
                                              None if as_planes else out.data_ptr(), out.data_ptr() if as_planes else None, C_, int(chunk_major),
                                              ops._stream()))
        c, rate = out, rate * s
    return c


def cascade_outs(pl, frames, C_, dev, want_planes):
    """A buffer per stage for `cascade` on [frames, C_]: fp32, the last one the planes of the result where wanted"""
    rows = [frames * int(r) for r in np.cumprod(pl.cfg["upsample_scales"])]
    return [torch.empty(r, C_, device=dev) for r in rows[:-1]] + [ops.planes_empty(rows[-1], C_, dev) if want_planes else torch.empty(rows[-1], C_, device=dev)]


def colour_basis(g):
    """e[g][c] = (g mod 5 == c), [frames, 8], of the frame numbers g: the upsampling network's response to it gives the coefficients of the
    frame-rate auxiliary term"""
    return (g[:, None] % 5 == torch.arange(8, device=g.device)[None, :]).to(torch.float32).contiguous()


def aux_term(pl, colour, frame_utt, utt_off, frames, chunk_major, stages, kp, cfull, cfull_p, pt_a, pt_b):
    """The auxiliary term of every block at frame rate (fcl_pwg_layer_t.kp): the upsampling network is linear and a sample of frame f sees frames
    f-2 .. f+2 only, so conv1x1_aux(upsample(c))[m] = sum_g k[m][g] (W_aux c_in[g]).  k (-> kp, coefficient lines [M]) is the network's response,
    utterance edges included, to the colour basis; cfull holds c_in in rows [16, 16 + frames) of zeros, and the projections W_aux c_in^T of all
    blocks are gate-row major over frames: line q of pt_a = frames [32q, 32q + 32), of pt_b = frames [32q - 16, 32q + 16)."""
    lib, s = _lib.load(), ops._stream()
    kc = cascade(pl, colour, frame_utt, utt_off, frames, chunk_major, stages)
    _lib.check(lib.fcl_pwg_aux_coeff(kc.data_ptr(), frames * pl.hop, pl.hop, frames, kp.data_ptr(), s))
    n, rows, w = cfull.shape[0] - 16, pl.w_aux_all_p.shape[0], pl.w_aux_all_p
    _lib.check(lib.fcl_pack_planes(cfull.data_ptr(), cfull.stride(0), cfull.shape[0], pl.A, cfull_p.data_ptr(), s))
    for src, pt in ((cfull_p[16:], pt_a), (cfull_p, pt_b)):
        _lib.check(lib.fcl_linear_planes_fwd(w.data_ptr(), w.shape[1] // 64, src.data_ptr(), None, None, n, pt.data_ptr(), rows, n, pl.A, ops.ACT_NONE, s))


def layer_chain(pl, M, seg_lo, seg_hi, xp, gp, skips, aux, x=None, unfused=None):
    """The descriptors of the residual blocks on M rows.  aux: (kp, pt_a, pt_b, ld_pt) of the frame-rate auxiliary term, or the planes cp of the
    upsampled features.  The one-launch blocks ping-pong between xp and gp; unfused = (z, o) workspaces selects the three-launch block, which
    updates fp32 x and xp in place and keeps the gate's planes in gp."""
    layers, R = [], pl.R
    p_in, p_out = xp.data_ptr(), gp.data_ptr()
    for l, L in enumerate(pl.layers):
        a = _lib.PwgLayer()
        a.m, a.r, a.aux, a.ksize, a.dilation, a.first_layer = M, R, pl.A, pl.k, L["dilation"], int(l == 0)
        a.seg_lo, a.seg_hi = seg_lo, seg_hi
        a.x, a.xp = None if x is None else x.data_ptr(), p_in
        a.w_conv_p, a.b_conv, a.w_aux_p = L["w_conv_p"].data_ptr(), L["b_conv"].data_ptr(), L["w_aux_p"].data_ptr()
        if isinstance(aux, tuple):
            kp, pt_a, pt_b, ld_pt = aux
            row0 = l * 2 * R * ld_pt * 64  # this block's gate rows of the stacked projection (int16 elements)
            a.kp, a.pt_a, a.pt_b = kp.data_ptr(), pt_a.data_ptr() + 2 * row0, pt_b.data_ptr() + 2 * row0
            a.ld_pt, a.hop = ld_pt, pl.hop
        else:
            a.cp = aux.data_ptr()
        a.w_os_p, a.b_os, a.skips = L["w_os_p"].data_ptr(), L["b_os"].data_ptr(), skips.data_ptr()
        if unfused is None:
            a.xp_out = p_out
            p_in, p_out = p_out, p_in
        else:
            a.z, a.gp, a.o = unfused[0].data_ptr(), p_out, unfused[1].data_ptr()
        layers.append(a)
    return layers


class CapacitySynth(object):
    """The generator in CAPACITY form: every buffer, index map and grid is sized once for `batch` utterance slots and `frames_cap` mel frames; what is
    live comes from the device (the synthesis pass's frame starts), so `run` derives no host value from the data, allocates nothing and is
    capturable in a hipGraph behind the synthesis pass (engine.SpeechRunner).  The sample-rate launches (noise, first_conv, the 30 blocks, the
    last stage, the PCM conversion) do no work past the live samples; the frame-rate launches and the 8-column coefficient cascade run over the
    capacity (1/256 of the rows, resp. 32 of ~1000 bytes per sample).  A live sample is computed exactly as `synthesize_packed` computes it on
    the same packed rows: same tiles, same frame windows, same absolute rows, same noise counter.

    Memory: 1082 bytes per capacity sample measured on the default path (two x plane buffers 2 x 256 B, the fp32 skip accumulator 256 B, coefficient
    lines 128 B, projected features 2 x 60 B, cascade ~43 B, bounds 8 B, z / wav / pcm 10 B), i.e. ~275 KB per capacity frame at hop 256 -- `nbytes`
    is the exact figure of an instance; FCL_PWG_AUX_FRAME_RATE=0 holds planes of the upsampled features instead (~1.35 KB per sample).
    Only the one-launch block geometry (fused_block(plan), 64 skip channels, hop a multiple of 128) has a capacity form: anything else raises FclError
    and callers keep the two-step route (synthesis, frames() on the host, synthesize_packed)."""

    def __init__(self, gen, batch, frames_cap, seed=0):
        pl = self.plan = gen.plan
        self.gen, self.B, self.frames_cap, self.seed = gen, int(batch), int(frames_cap), int(seed) & 0xFFFFFFFF
        dev = pl.device
        if not fused_block(pl) or pl.S != 64 or pl.hop % 128:
            raise _lib.FclError("fcl-taco2_amd: the capacity vocoder is built for the one-launch block (64 residual / skip channels, kernel 3, <= 96 auxiliary "
                                "channels, FCL_PWG_FUSED not 0) and a hop that is a multiple of 128; use synthesize_packed for this generator")
        if not aux_frame_rate(pl) and pl.A <= 64:
            raise _lib.FclError("fcl-taco2_amd: the capacity vocoder from upsampled planes (FCL_PWG_AUX_FRAME_RATE=0) needs more than 64 auxiliary channels")
        check_capacity(self.B, self.frames_cap, pl.hop)
        self.ctx = ctx = int(pl.cfg["aux_context_window"])
        self.aux_fr = aux_frame_rate(pl)
        F, R, A, hop = self.frames_cap, pl.R, pl.A, pl.hop
        self.pad_cap, self.M = capacity_sizes(self.B, F, ctx, hop)
        M = self.M
        with torch.cuda.device(dev):
            before = torch.cuda.memory_allocated(dev)
            i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
            f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
            self.maps = dict(pad_idx=i32(self.pad_cap), lo=i32(self.pad_cap), hi=i32(self.pad_cap), keep=i32(F), frame_utt=i32(F), utt_off=i32(self.B + 2),
                             seg_lo=i32(M), seg_hi=i32(M))
            self.live = i32(4)
            self.z, self.wav, self.skips = f32(M), f32(M), f32(M, R)
            self.pcm = torch.empty(M, dtype=torch.int16, device=dev)
            self.xp = torch.empty(R // 32, M, 64, dtype=torch.int16, device=dev)  # chunk-major planes; the blocks ping-pong between xp and gp
            self.gp = torch.empty(R // 32, M, 64, dtype=torch.int16, device=dev)
            self.c_pad, self.c_conv = f32(self.pad_cap, A), f32(self.pad_cap, A)
            self._stages = cascade_outs(pl, F, 8, dev, False) if self.aux_fr else cascade_outs(pl, F, A, dev, True)  # (chunk-major planes)
            if self.aux_fr:
                g = torch.arange(F, device=dev)  # (alive until `nbytes` is read below, which has always counted it)
                self.colour = colour_basis(g)
                self.kp = ops.planes_empty(M, 32, dev)
                self.ld_pt = (F + 16 + 31) // 32
                n = self.ld_pt * 32
                self.cfull = torch.zeros(16 + n, A, device=dev)  # rows [16, 16 + F) are rewritten by every run, the rest stays zero
                self.cfull_p = ops.planes_empty(16 + n, A, dev)
                rows = pl.w_aux_all_p.shape[0]
                self.pt_a, self.pt_b = ops.planes_empty(rows, n, dev), ops.planes_empty(rows, n, dev)
                self.c_in = self.cfull[16 : 16 + F]
            else:
                self.c_in = f32(F, A)
            for t_ in (self.xp, self.gp, self.kp if self.aux_fr else self._stages[-1]):
                assert t_.data_ptr() % 128 == 0
            self.nbytes = torch.cuda.memory_allocated(dev) - before
            # the block descriptors: every pointer is static
            self._layers = layer_chain(pl, M, self.maps["seg_lo"].data_ptr(), self.maps["seg_hi"].data_ptr(), self.xp, self.gp, self.skips,
                                       (self.kp, self.pt_a, self.pt_b, self.ld_pt) if self.aux_fr else self._stages[-1])
            # eager warm-up on an empty batch: the library's one-time setup (dynamic-LDS opt-ins) must not happen inside a capture
            st = i32(1)
            self.run(torch.zeros(1, A, device=dev), i32(self.B + 1), st)
            torch.cuda.current_stream(dev).synchronize()

    def _cascade(self, c):
        return cascade(self.plan, c, self.maps["frame_utt"], self.maps["utt_off"], self.frames_cap, True, self._stages)

    def run(self, mel_rows_cap, utt_frame0_dev, status, seed_dev=None, draw_noise=True):
        """Enqueue the whole generator + the PCM conversion on the current stream.  mel_rows_cap: [rows, aux] float32 device tensor whose first
        utt_frame0[B] rows are the batch's packed mel frames (later rows are never read as features); utt_frame0_dev: int32 [B + 1] on the device;
        status: the pass's int32 status word (FCL_STATUS_VOCODER_CAP / FCL_STATUS_PCM_NONFINITE are OR-ed into it; a word that is already set
        makes this pass generate nothing); seed_dev: optional int32 device word added to the seed (a graph advances it per replay);
        draw_noise=False: `self.z` already holds the noise.  Results: self.pcm (int16) and self.wav (float32), live samples [0, self.live[1])."""
        pl, lib, mp = self.plan, _lib.load(), self.maps
        check_run_args(mel_rows_cap, utt_frame0_dev, status, pl.A, self.B)
        s, live = ops._stream(), self.live.data_ptr()
        chk, F, M = _lib.check, self.frames_cap, self.M
        chk(lib.fcl_pwg_maps_build(utt_frame0_dev.data_ptr(), status.data_ptr(), self.B, F, self.ctx, pl.hop, mp["pad_idx"].data_ptr(), mp["lo"].data_ptr(),
                                   mp["hi"].data_ptr(), mp["keep"].data_ptr(), mp["frame_utt"].data_ptr(), mp["utt_off"].data_ptr(), mp["seg_lo"].data_ptr(),
                                   mp["seg_hi"].data_ptr(), live, s))
        # feature side at frame rate, over the capacity: replicate padding (dead rows zero) + conv_in ('valid' = 'same' on the interior)
        chk(lib.fcl_pwg_gather_pad(mel_rows_cap.data_ptr(), mel_rows_cap.shape[0], mp["pad_idx"].data_ptr(), live, self.pad_cap, pl.A, self.c_pad.data_ptr(), s))
        k, cout, cin = pl.conv_in.shape
        chk(lib.fcl_conv1d_fwd(self.c_pad.data_ptr(), pl.conv_in.data_ptr(), None, mp["lo"].data_ptr(), mp["hi"].data_ptr(), None, self.c_conv.data_ptr(),
                               self.pad_cap, cin, cout, k, ops.ACT_NONE, s))
        chk(lib.fcl_gather_rows_fwd(self.c_conv.data_ptr(), mp["keep"].data_ptr(), self.c_in.data_ptr(), None, F, pl.A, s))
        if self.aux_fr:
            aux_term(pl, self.colour, mp["frame_utt"], mp["utt_off"], F, True, self._stages, self.kp, self.cfull, self.cfull_p, self.pt_a, self.pt_b)
        else:
            self._cascade(self.c_in)
        if draw_noise:
            chk(lib.fcl_pwg_noise_cap(self.z.data_ptr(), M, self.seed, None if seed_dev is None else seed_dev.data_ptr(), live, s))
        chk(lib.fcl_pwg_first_conv_cap(self.z.data_ptr(), pl.first_w.data_ptr(), pl.first_b.data_ptr(), self.xp.data_ptr(), M, pl.R, live, s))
        for a in self._layers:
            chk(lib.fcl_pwg_layer_cap_fwd(C.byref(a), live, s))
        chk(lib.fcl_pwg_last_cap_fwd(self.skips.data_ptr(), math.sqrt(1.0 / len(pl.layers)), pl.last_w1p.data_ptr(), pl.last_b1.data_ptr(), pl.last_w2.data_ptr(),
                                     pl.last_b2, self.wav.data_ptr(), M, pl.S, live, s))
        chk(lib.fcl_pcm16_fwd(self.wav.data_ptr(), self.pcm.data_ptr(), M, live, status.data_ptr(), s))
        return self.pcm


class Generator(object):
    """What the vocoder families share: mel -> waveform.  `synthesize(mels)` is the batched entry, `synthesize_packed` (the family's own) takes
    utterances already packed row-wise, `inference(c, x=None)` mirrors the published single-utterance call."""

    def __init__(self, plan):
        self.plan = plan

    def samples_of(self, frames):
        """samples of an utterance of `frames` mel frames"""
        return int(frames) * self.plan.hop

    def check_lens(self, lens, ids=None):
        """a family's own refusal of utterance lengths (none here)"""

    def synthesize(self, mels, noise=None, seed=0, return_intermediates=False, **kw):
        """mels: list of [T'_i, aux] float tensors / arrays.  noise: optional list of [T'_i * hop] arrays for a family that draws noise (else drawn
        on the device from `seed`).  Returns a list of float32 device tensors, samples_of(T'_i) samples each ([samples, out] for out > 1)."""
        dev = self.plan.device
        with torch.cuda.device(dev):
            lens = [int(m.shape[0]) for m in mels]
            mel_rows = torch.cat([torch.as_tensor(m, dtype=torch.float32).to(dev) for m in mels]).contiguous()
            return self.synthesize_packed(mel_rows, lens, noise, seed, return_intermediates, **kw)

    def inference(self, c, x=None):
        """c [T', aux] (x: optional noise [T' * hop]) -> waveform [samples, out_channels]."""
        return self.synthesize([c], None if x is None else [x])[0].reshape(-1, getattr(self.plan, "out_channels", 1))

    def _packed_lens(self, mel_rows, lens, ids=None):
        """the frame counts as ints, after what every synthesize_packed refuses"""
        lens = [int(n) for n in lens]
        if not lens or min(lens) < 1:
            raise _lib.FclError("fcl-taco2_amd: empty mel")
        self.check_lens(lens, ids)
        if mel_rows.dim() != 2 or mel_rows.shape[1] != self.plan.A or mel_rows.shape[0] != sum(lens):
            raise _lib.FclError("fcl-taco2_amd: expected [%d, %d] mel rows, got %r" % (sum(lens), self.plan.A, tuple(mel_rows.shape)))
        return lens

    @staticmethod
    def _results(outs, intermediates, flat, return_intermediates, return_flat):
        res = (outs,) + ((intermediates,) if return_intermediates else ()) + ((flat,) if return_flat else ())
        return res[0] if len(res) == 1 else res


class ParallelWaveGANGenerator(Generator):
    """The Parallel WaveGAN generator on a PWGPlan."""

    def __init__(self, plan):
        Generator.__init__(self, plan)
        self._maps_cache = {}

    def capacity_synth(self, batch, frames_cap, seed=0):
        """The capacity form of this generator for `batch` utterance slots and `frames_cap` mel frames (what engine.SpeechRunner captures)."""
        return CapacitySynth(self, batch, frames_cap, seed=seed)

    # ---- integer index maps of a batch shape (host-built once per tuple of utterance lengths, cached) -------------------------------------------
    def _maps(self, lens):
        key = tuple(lens)
        hit = self._maps_cache.get(key)
        if hit is not None:
            cur = torch.cuda.current_stream(self.plan.device)
            cur.wait_event(hit["ready"])  # built on another stream, possibly: order this one behind it
            if cur.cuda_stream not in hit["streams"]:  # ... and tell the caching allocator that this stream reads the maps too: an eviction while
                hit["streams"].add(cur.cuda_stream)    # its kernels are in flight must not hand the blocks back to the building stream
                for v in hit.values():
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(cur)
            return hit
        pl, dev = self.plan, self.plan.device
        ctx = pl.cfg["aux_context_window"]
        lens_np = np.asarray(lens, dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens_np)]).astype(np.int64)
        pad_idx, lo, hi, keep = [], [], [], []
        base = 0
        for u, n in enumerate(lens):  # padded utterance = frames clamp(-ctx .. n-1+ctx); conv_in is 'valid', i.e. 'same' evaluated on the interior
            pad_idx.append(offs[u] + np.clip(np.arange(-ctx, n + ctx), 0, n - 1))
            lo.append(np.full(n + 2 * ctx, base))
            hi.append(np.full(n + 2 * ctx, base + n + 2 * ctx))
            keep.append(np.arange(base + ctx, base + ctx + n))
            base += n + 2 * ctx
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        m = dict(offs=offs, pad_idx=i32(np.concatenate(pad_idx)), lo=i32(np.concatenate(lo)), hi=i32(np.concatenate(hi)), keep=i32(np.concatenate(keep)),
                 frame_utt=i32(np.repeat(np.arange(len(lens)), lens_np)), utt_off=i32(offs))
        s_off = torch.from_numpy(offs * pl.hop).to(dev)
        reps = torch.from_numpy(lens_np * pl.hop).to(dev)
        m["seg_lo"] = torch.repeat_interleave(s_off[:-1], reps).to(torch.int32)  # sample range of each row's utterance (integers only)
        m["seg_hi"] = torch.repeat_interleave(s_off[1:], reps).to(torch.int32)
        m["ready"] = torch.cuda.Event()  # the cached maps may be used from other streams later: those wait for this event (no host synchronisation:
        m["ready"].record(torch.cuda.current_stream(dev))  # a driver that sees a new batch shape every call keeps its batches pipelined)
        m["streams"] = {torch.cuda.current_stream(dev).cuda_stream}
        if len(self._maps_cache) >= 4:
            self._maps_cache.clear()
        self._maps_cache[key] = m
        return m

    # ---- feature side: replicate padding + conv_in at frame rate, then 4 x (stretch + smoothing) to sample rate --------------------------------
    def _conv_in(self, mel_rows, mp):
        """replicate padding + conv_in at frame rate -> [sum T', A]"""
        c_pad = ops.gather_rows(mel_rows, mp["pad_idx"])
        c_in = ops.conv1d(c_pad, self.plan.conv_in, None, mp["lo"], mp["hi"])
        return ops.gather_rows(c_in, mp["keep"])

    def _cascade(self, c, mp, want_planes, chunk_major=False):
        """The 4 x (stretch + smoothing) stages on c [frames, C] (C % 4 == 0): planes of the result (want_planes) or the fp32 result."""
        frames = int(mp["offs"][-1])
        return cascade(self.plan, c, mp["frame_utt"], mp["utt_off"], frames, chunk_major, cascade_outs(self.plan, frames, c.shape[1], self.plan.device, want_planes))

    def _upsample(self, mel_rows, mp, chunk_major):
        return self._cascade(self._conv_in(mel_rows, mp), mp, True, chunk_major)

    def _aux_frame_rate(self, mel_rows, mp):
        """The operands of aux_term at the batch's size.  Returns (coefficient lines [M], planes of W_aux c_in^T for all blocks in the two window
        alignments, lines per row)."""
        pl, dev = self.plan, self.plan.device
        frames = int(mp["offs"][-1])
        e, stages = colour_basis(torch.arange(frames, device=dev)), cascade_outs(pl, frames, 8, dev, False)
        kp = ops.planes_empty(frames * pl.hop, 32, dev)
        ld_pt = (frames + 16 + 31) // 32
        n, rows = ld_pt * 32, pl.w_aux_all_p.shape[0]
        cfull = torch.zeros(16 + n, pl.A, device=dev)
        cfull[16 : 16 + frames] = self._conv_in(mel_rows, mp)
        cfull_p, pt_a, pt_b = ops.planes_empty(16 + n, pl.A, dev), ops.planes_empty(rows, n, dev), ops.planes_empty(rows, n, dev)
        aux_term(pl, e, mp["frame_utt"], mp["utt_off"], frames, False, stages, kp, cfull, cfull_p, pt_a, pt_b)
        return kp, pt_a, pt_b, ld_pt

    def synthesize_packed(self, mel_rows, lens, noise=None, seed=0, return_intermediates=False, return_flat=False):
        """The same on utterances already packed row-wise ([sum T', aux] device tensor, e.g. engine.run's output) with their frame counts.
        return_flat: also return the one [sum T' * hop] buffer the per-utterance waveforms are slices of (utterances back to back), as the last result."""
        pl, dev = self.plan, self.plan.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            lens = self._packed_lens(mel_rows, lens)
            if sum(lens) * pl.hop >= 2 ** 31:  # before any int32 index map is built or any kernel launched with the overflowing sizes
                raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples in one vocoder batch")
            mp = self._maps(lens)
            offs = mp["offs"]
            M, R = int(offs[-1]) * pl.hop, pl.R
            fused = fused_block(pl)
            # the one-launch block reads chunk-major planes of the upsampled features (contiguous rows per 32-column chunk)
            aux = self._aux_frame_rate(mel_rows, mp) if aux_frame_rate(pl) else self._upsample(mel_rows, mp, fused)
            if noise is None:
                z = torch.empty(M, device=dev)
                _lib.check(lib.fcl_pwg_noise(z.data_ptr(), M, seed & 0xFFFFFFFF, ops._stream()))
            else:
                z = torch.cat([torch.as_tensor(n_, dtype=torch.float32).reshape(-1).to(dev) for n_ in noise]).contiguous()
                if z.numel() != M:
                    raise _lib.FclError("fcl-taco2_amd: noise must hold T' * %d samples per utterance" % pl.hop)
            seg_lo, seg_hi = mp["seg_lo"], mp["seg_hi"]
            # the one-launch blocks carry x as planes only; fp32 x is then just the workspace of the general last stage (not needed for 64 channels)
            x = None if fused and pl.S == 64 else torch.empty(M, R, device=dev)
            xp = ops.planes_empty(M, R, dev)
            _lib.check(lib.fcl_pwg_first_conv(z.data_ptr(), pl.first_w.data_ptr(), pl.first_b.data_ptr(), None if fused else x.data_ptr(), xp.data_ptr(),
                                              M, R, int(fused), ops._stream()))
            skips = torch.empty(M, R, device=dev)
            gp = ops.planes_empty(M, R, dev)  # unfused: the gate's planes; fused: the second x buffer (blocks ping-pong between xp and gp)
            unfused = None if fused else (torch.empty(M, 2 * R, device=dev), torch.empty(M, 2 * R, device=dev))
            taps = []
            for a in layer_chain(pl, M, seg_lo.data_ptr(), seg_hi.data_ptr(), xp, gp, skips, aux, x, unfused):
                _lib.check(lib.fcl_pwg_layer_fwd(C.byref(a), ops._stream()))
                if fused:
                    xp, gp = gp, xp
                if return_intermediates:
                    taps.append(unpack_planes(xp, R, chunk_major=True) if fused else x.clone())
            wav = torch.empty(M, device=dev)
            _lib.check(lib.fcl_pwg_last_fwd(skips.data_ptr(), math.sqrt(1.0 / len(pl.layers)), pl.last_w1p.data_ptr(), pl.last_b1.data_ptr(),
                                            pl.last_w2.data_ptr(), pl.last_b2, gp.data_ptr(), None if x is None else x.data_ptr(), wav.data_ptr(), M, pl.S,
                                            ops._stream()))
            outs = [wav[int(offs[i]) * pl.hop : int(offs[i + 1]) * pl.hop] for i in range(len(lens))]
            return self._results(outs, dict(z=z, taps=taps, skips=skips, seg=(seg_lo, seg_hi)), wav, return_intermediates, return_flat)
