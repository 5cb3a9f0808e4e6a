"""HiFi-GAN generator on the HIP path: mel [T', 80] -> waveform [T' * 256] (csrc/hifigan.hip).

The second generator family `parallel-wavegan-decode` (inference_student.sh:20-23) selects by `generator_type`, built from the published
architecture (kan-bayashi/ParallelWaveGAN `HiFiGANGenerator`, v1 / LJSpeech; restated in float64 in tests/hifigan_ref.py -- no upstream source,
checkpoint or vector here: parity unpinned).  State-dict names are that package's, so its checkpoints (`{"model": {"generator": ...}}`, with or
without weight norm) load here; the loader is strict about names and shapes.

Batched: utterances are concatenated row-major (rows = samples at the stage's rate, channels-last); every convolution and the transposed
convolutions see zeros outside their own utterance.  The generator is deterministic: `seed` / `noise` are accepted and unused.  No CPU fallback;
needs the pre-split path (FCL_PRECISION / FCL_PLANES not 0).  No capacity form: engine.SpeechRunner refuses this generator and tts.synthesize takes
its two-step route for every batch."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .vocoder import fold_weight_norm

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


class HiFiGANPlan(object):
    """Device-resident, GEMM-ready weights of one generator: tap-major P32 planes of every convolution, packed once."""

    eager_only = True  # no capacity form: tts.synthesize keeps the two-step route, engine.SpeechRunner refuses

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


class HiFiGANGenerator(object):
    """mel -> waveform.  `synthesize(mels)` is the batched entry; `inference(c)` mirrors the published single-utterance call."""

    def __init__(self, plan):
        self.plan = plan

    def synthesize(self, mels, noise=None, seed=0, return_intermediates=False):
        """mels: list of [T'_i, in_channels] float tensors / arrays -> list of [T'_i * hop] float32 device tensors ([T'_i * hop, out] for out > 1)."""
        dev = self.plan.device
        with torch.cuda.device(dev):
            lens = [int(m.shape[0]) for m in mels]
            mel_rows = torch.cat([torch.as_tensor(m, dtype=torch.float32).to(dev) for m in mels]).contiguous()
            return self.synthesize_packed(mel_rows, lens, noise, seed, return_intermediates)

    def synthesize_packed(self, mel_rows, lens, noise=None, seed=0, return_intermediates=False, return_flat=False):
        """The same on utterances already packed row-wise ([sum T', in_channels] device tensor) with their frame counts.  return_intermediates: also a
        dict with `taps` = [input_conv's output, every stage's output c] (fp32).  return_flat: also the one buffer the waveforms are slices of."""
        pl, dev = self.plan, self.plan.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            lens = [int(n) for n in lens]
            if not lens or min(lens) < 1:
                raise _lib.FclError("fcl-taco2_amd: empty mel")
            if mel_rows.dim() != 2 or mel_rows.shape[1] != pl.A or mel_rows.shape[0] != sum(lens):
                raise _lib.FclError("fcl-taco2_amd: expected [%d, %d] mel rows, got %r" % (sum(lens), pl.A, tuple(mel_rows.shape)))
            F = sum(lens)
            if F * pl.hop >= 2 ** 30:
                raise _lib.FclError("fcl-taco2_amd: more than 2^30 samples in one vocoder batch")
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            frame_utt = torch.from_numpy(np.repeat(np.arange(len(lens)), lens).astype(np.int32)).to(dev)
            utt_off = torch.from_numpy(offs.astype(np.int32)).to(dev)
            fu, uo, s_ = frame_utt.data_ptr(), utt_off.data_ptr(), ops._stream()
            f32 = lambda r, c: torch.empty(r, c, device=dev, dtype=torch.float32)
            taps = []
            melp = ops.pack_planes(mel_rows.to(torch.float32).contiguous())
            a = _lib.HfgConv()
            a.m, a.cin, a.cout, a.ksize, a.dilation, a.rate, a.slope = F, pl.input["cin"], pl.input["cout"], pl.input["k"], 1, 1, pl.slope
            a.xp, a.wp, a.bias, a.frame_utt, a.utt_off = melp.data_ptr(), pl.input["wp"].data_ptr(), pl.input["b"].data_ptr(), fu, uo
            cp = ops.planes_empty(F, a.cout, dev)
            a.yp = cp.data_ptr()
            if return_intermediates:
                c0 = f32(F, a.cout)
                a.y = c0.data_ptr()
                taps.append(c0)
            _lib.check(lib.fcl_hfg_conv_fwd(C.byref(a), s_))
            rate, rows = 1, F
            for si, st in enumerate(pl.stages):
                last_stage = si == len(pl.stages) - 1
                tc = _lib.HfgTconv()
                tc.m_in, tc.cin, tc.cout, tc.stride, tc.ksize, tc.padding, tc.rate_in, tc.slope = rows, st["cin"], st["cout"], st["s"], st["ku"], \
                    tconv_padding(st["s"])[0], rate, pl.slope
                rows, rate, Cc = rows * st["s"], rate * st["s"], st["cout"]
                c, cpl = f32(rows, Cc), ops.planes_empty(rows, Cc, dev)
                tc.xp, tc.wp, tc.bias, tc.frame_utt, tc.utt_off, tc.y, tc.yp = cp.data_ptr(), st["wp"].data_ptr(), st["b"].data_ptr(), fu, uo, c.data_ptr(), \
                    cpl.data_ptr()
                _lib.check(lib.fcl_hfg_tconv_fwd(C.byref(tc), s_))
                xb, cs = f32(rows, Cc), f32(rows, Cc)
                pa, pb, csp = ops.planes_empty(rows, Cc, dev), ops.planes_empty(rows, Cc, dev), ops.planes_empty(rows, Cc, dev)
                tp = ops.planes_empty(rows, Cc, dev) if Cc not in (32, 64, 128) else None
                nk = len(st["blocks"])
                for j, units in enumerate(st["blocks"]):
                    x_in, xp_in, xp_out = c, cpl, pa
                    for d, U in enumerate(units):
                        last = d == len(units) - 1
                        u = _lib.HfgUnit()
                        u.m, u.c, u.ksize, u.dilation, u.rate, u.first, u.last = rows, Cc, U["k"], U["dilation"], rate, int(j == 0), int(last)
                        u.slope, u.cs_scale, u.csp_slope = pl.slope, 1.0 / nk, OUT_SLOPE if last_stage else pl.slope
                        u.xp, u.x, u.w1p, u.b1, u.w2p, u.b2 = xp_in.data_ptr(), x_in.data_ptr(), U["w1p"].data_ptr(), U["b1"].data_ptr(), U["w2p"].data_ptr(), \
                            U["b2"].data_ptr()
                        u.frame_utt, u.utt_off = fu, uo
                        if last:
                            u.cs, u.csp = cs.data_ptr(), csp.data_ptr() if j == nk - 1 else None
                        else:
                            u.x_out, u.xp_out = xb.data_ptr(), xp_out.data_ptr()
                        u.tp = None if tp is None else tp.data_ptr()
                        _lib.check(lib.fcl_hfg_unit_fwd(C.byref(u), s_))
                        x_in, xp_in, xp_out = xb, xp_out, (pb if xp_out is pa else pa)
                cp = csp
                if return_intermediates:
                    taps.append(cs)
            M, oc = rows, pl.out_channels
            flat = torch.empty(M * oc, device=dev, dtype=torch.float32)  # the per-utterance waveforms are slices of this one buffer
            _lib.check(lib.fcl_hfg_out_fwd(cp.data_ptr(), pl.out_w.data_ptr(), pl.out_b.data_ptr(), fu, uo, rate, flat.data_ptr(), M, pl.c_last, oc,
                                           pl.cfg["kernel_size"], s_))
            outs = [flat[int(offs[i]) * pl.hop * oc : int(offs[i + 1]) * pl.hop * oc] for i in range(len(lens))]
            if oc > 1:
                outs = [o.reshape(-1, oc) for o in outs]
            if return_intermediates:
                res = (outs, dict(taps=taps, lens=lens))
                return res + (flat,) if return_flat else res
            return (outs, flat) if return_flat else outs

    def inference(self, c, x=None):
        """HiFiGANGenerator.inference(c): c [T', in_channels] -> waveform [T' * hop, out_channels]."""
        return self.synthesize([c])[0].reshape(-1, self.plan.out_channels)
