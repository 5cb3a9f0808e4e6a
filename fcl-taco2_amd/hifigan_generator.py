"""The HiFi-GAN generator in its training form: input_conv and the upsampling stages -- the transposed convolutions and the multi-receptive-field
residual blocks -- forward (pre-activations kept) and backward on the HIP path (the hft_* kernels of csrc/hifigan_train.hip), under an
nn.Module with the parallel_wavegan package's constructor arguments and parameter names.

    gen = TrainableHiFiGANGenerator().to("cuda:0")
    gen.load_state_dict(torch.load("checkpoint.pkl"))          # either name form, or the whole checkpoint
    fake = gen(mel, lens)                                      # mel [B, 80, T'] -> [B, 1, T' * 256]
    mel_loss.MelSpectrogramLoss(...)(fake, real).backward()    # the stages run backward in HIP kernels; torch folds weight norm
    hifigan.HiFiGANPlan(gen.state_dict(), "cuda:0")            # the inference generator takes the trained weights as they are

The launches' contract is stated in include/fcl_hip.h "HiFi-GAN generator, training form" and restated in float64 numpy in tests/hfgt_ref.py.
Activations are float32, channel-last [rows, C], the batch packed with the utterances back to back; rows are samples at the stage's own rate.  Kept per
stage: its input c, the transposed convolution's output u and every unit's xt and x' (pre-activations only).  One arithmetic mode (exact fp32).  The output
end (LeakyReLU at hifigan.OUT_SLOPE, output_conv, tanh) is either torch operations on the unpacked batch (forward(output_end="torch"), the default) or
the hfe_* kernels of csrc/hifigan_end.hip on the packed rows (output_end="hip"; DESIGN.md §6s, tests/hfge_ref.py).  No CPU fallback."""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib, hifigan, ops
from .pwg_common import Maps, _Conv, _Module, _norm

CONV_FWD, CONV_DX, CONV_DW = "hft_conv_kernel", "hft_conv_dx_kernel", ("hft_dw_kernel", "hft_dw_reduce_kernel")
TCONV_FWD, TCONV_DX, TCONV_DW = "hft_tconv_kernel", "hft_tconv_dx_kernel", ("hft_tconv_dw_kernel", "hft_dw_reduce_kernel")
SUM_KERNEL = "hft_sum_kernel"
END_FWD, END_DX, END_DW = "hfe_fwd_kernel", "hfe_dx_kernel", ("hfe_dw_kernel", "hfe_dw_reduce_kernel")
OUTPUT_ENDS = ("torch", "hip")
KERNEL_SIZES, MAX_WIDTH, MAX_BLOCKS = (3, 5, 7, 11), 512, 4


def check_training(cfg):
    """cfg: hifigan.config's result.  Whatever the training kernels do not cover is refused by the parameter's name, before any device call."""
    bad = lambda name, got, want: ValueError("fcl-taco2_amd: HiFi-GAN generator: %s=%r is not supported on the HIP training path (%s)" % (name, got, want))
    width = lambda v: isinstance(v, int) and 16 <= v <= MAX_WIDTH and v % 16 == 0
    if not width(cfg["in_channels"]):
        raise bad("in_channels", cfg["in_channels"], "a multiple of 16 from 16 to %d" % MAX_WIDTH)
    if not (isinstance(cfg["out_channels"], int) and 1 <= cfg["out_channels"] <= 4):
        raise bad("out_channels", cfg["out_channels"], "1 to 4")
    n = len(cfg["upsample_scales"])
    if not width(cfg["channels"]) or cfg["channels"] % (16 << n):
        raise bad("channels", cfg["channels"], "a multiple of 16 x 2^stages up to %d: every stage's width a multiple of 16" % MAX_WIDTH)
    if cfg["kernel_size"] not in KERNEL_SIZES:
        raise bad("kernel_size", cfg["kernel_size"], "3, 5, 7 or 11")
    if n < 1 or any(not 2 <= s <= 16 for s in cfg["upsample_scales"]):
        raise bad("upsample_scales", cfg["upsample_scales"], "at least one scale, each 2 to 16")
    if tuple(cfg["upsample_kernel_sizes"]) != tuple(2 * s for s in cfg["upsample_scales"]):
        raise bad("upsample_kernel_sizes", cfg["upsample_kernel_sizes"], "2 x the scale")
    if not 1 <= len(cfg["resblock_kernel_sizes"]) <= MAX_BLOCKS or any(k not in KERNEL_SIZES for k in cfg["resblock_kernel_sizes"]):
        raise bad("resblock_kernel_sizes", cfg["resblock_kernel_sizes"], "1 to %d sizes of 3, 5, 7 or 11" % MAX_BLOCKS)
    if len(cfg["resblock_dilations"]) != len(cfg["resblock_kernel_sizes"]) or any(d < 1 for ds in cfg["resblock_dilations"] for d in ds) or any(
            len(ds) < 1 for ds in cfg["resblock_dilations"]):
        raise bad("resblock_dilations", cfg["resblock_dilations"], "one non-empty list of positive dilations per kernel size")
    slope = cfg["nonlinear_activation_params"].get("negative_slope", 0.01)
    if not 0.0 <= slope < 1.0:
        raise bad("nonlinear_activation_params", cfg["nonlinear_activation_params"], "negative_slope in [0, 1)")
    return cfg


class StageMaps(object):
    """the packed batch's row tables at every rate: maps[0] on the frames, maps[i + 1] behind stage i; and the index that packs / unpacks a padded batch"""

    def __init__(self, frames, scales, device):
        self.frames, self.rates = [int(f) for f in frames], [1]
        for s in scales:
            self.rates.append(self.rates[-1] * int(s))
        self.maps = [Maps([f * r for f in self.frames], device) for r in self.rates]
        self.hop, self.n_utt, self.device, self._rows = self.rates[-1], len(self.frames), device, {}

    def rows(self, T, rate):
        """int64 on the device: where the pack's rows (at `rate` rows per frame) sit in a padded batch's [B T rate] rows"""
        if (T, rate) not in self._rows:
            m = torch.arange(T * rate).unsqueeze(0) < torch.tensor(self.frames).unsqueeze(1) * rate
            self._rows[(T, rate)] = torch.nonzero(m.reshape(-1))[:, 0].to(self.device)
        return self._rows[(T, rate)]


class TrainingPlan(object):
    """Per-stage geometry and the sizes of what a pass over a batch needs"""

    def __init__(self, device="cuda:0", **config):
        known = {k: v for k, v in config.items() if k in hifigan.CONFIG}
        self.cfg = cfg = check_training(hifigan.config(known))
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: TrainingPlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)
        self.slope = float(cfg["nonlinear_activation_params"].get("negative_slope", 0.01))
        self.scales, self.nk = cfg["upsample_scales"], len(cfg["resblock_kernel_sizes"])
        self.blocks = list(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilations"]))
        self.widths = [cfg["channels"] >> i for i in range(len(self.scales) + 1)]
        self.in_channels, self.kernel_size = cfg["in_channels"], cfg["kernel_size"]
        self.hop = 1
        for s in self.scales:
            self.hop *= s

    def stage_params(self):
        """parameters per stage in the autograd function's order: the transposed convolution's two, then (w1, b1, w2, b2) per block and unit"""
        return 2 + 4 * sum(len(d) for _, d in self.blocks)

    def kept_shapes(self, maps, stage):
        """(u, per block per unit (xt, x'), the stage's output), all [rows behind the stage, its width]"""
        shp = (maps.maps[stage + 1].samples, self.widths[stage + 1])
        return shp, [[(shp, shp) for _ in dils] for _, dils in self.blocks], shp

    def kept_bytes(self, maps):
        units = sum(len(d) for _, d in self.blocks)
        return 4 * sum(maps.maps[i + 1].samples * self.widths[i + 1] * (2 + 2 * units) for i in range(len(self.scales)))

    def workspace_floats(self, maps):
        """the largest weight gradient's partials over every stage (and input_conv)"""
        lib = _lib.load()
        need = lib.fcl_hft_workspace_bytes(maps.maps[0].samples, self.in_channels, self.widths[0], self.kernel_size, 1)
        for i, s in enumerate(self.scales):
            need = max(need, lib.fcl_hft_workspace_bytes(maps.maps[i].samples, self.widths[i], self.widths[i + 1], 2 * s, s))
            for k, _ in self.blocks:
                need = max(need, lib.fcl_hft_workspace_bytes(maps.maps[i + 1].samples, self.widths[i + 1], self.widths[i + 1], k, 1))
        return need // 4

    def dweight_shapes(self, stage):
        """(dwt [2 s, cin, cout], dbt [cout], per block per unit (dw1 [k, C, C], db1 [C], dw2, db2)) in the kernels' layout"""
        ci, co, s = self.widths[stage], self.widths[stage + 1], self.scales[stage]
        return (2 * s, ci, co), (co,), [[((k, co, co), (co,), (k, co, co), (co,)) for _ in dils] for k, dils in self.blocks]


def _f(v):
    return v.detach().to(torch.float32)


def pack_conv(w):
    """torch Conv1d weight (cout, cin, k) -> (forward [k, cin, cout], input-gradient [k, cout, cin] with the taps reversed)"""
    w = _f(w)
    return w.permute(2, 1, 0).contiguous(), w.flip(2).permute(2, 0, 1).contiguous()


def pack_tconv(w, s):
    """torch ConvTranspose1d weight (cin, cout, 2 s) -> (forward [s, 2, cin, cout]: phase ph holds W[:, :, ph + s] then W[:, :, ph]; input-gradient
    [2 s, cout, cin])"""
    w = _f(w)
    t = w.permute(2, 0, 1)  # [2 s, cin, cout]
    return torch.stack([t[s:], t[:s]], dim=1).contiguous(), w.permute(2, 1, 0).contiguous()


def pack_weights(plan, stage, params):
    """one stage's plain torch parameters in stage_params order -> the kernels' forms.  Permutations only; nothing here is differentiated."""
    s = plan.scales[stage]
    tf, tdx = pack_tconv(params[0], s)
    out, at = dict(tw=tf, tb=_f(params[1]).contiguous(), tw_dx=tdx, units=[]), 2
    for _, dils in plan.blocks:
        blk = []
        for _ in dils:
            w1, b1, w2, b2 = params[at : at + 4]
            at += 4
            (f1, x1), (f2, x2) = pack_conv(w1), pack_conv(w2)
            blk.append(dict(w1=f1, b1=_f(b1).contiguous(), w2=f2, b2=_f(b2).contiguous(), w1_dx=x1, w2_dx=x2))
        out["units"].append(blk)
    return out


def unpack_dweights(dwt, dbt, units):
    """the kernels' gradient forms of one stage -> torch's, in stage_params order"""
    out = [dwt.permute(1, 2, 0).contiguous(), dbt]
    for blk in units:
        for dw1, db1, dw2, db2 in blk:
            out += [dw1.permute(2, 1, 0).contiguous(), db1, dw2.permute(2, 1, 0).contiguous(), db2]
    return out


def conv_args(maps, cin, cout, k, dil, slope, lrelu=0, **ptr):
    a = _lib.HftConv()
    a.rows, a.cin, a.cout, a.ksize, a.dilation, a.lrelu, a.slope = maps.samples, cin, cout, k, dil, int(lrelu), slope
    a.seg_lo, a.seg_hi = maps.seg_lo.data_ptr(), maps.seg_hi.data_ptr()
    for n, v in ptr.items():
        if n == "workspace" and v is not None:
            a.workspace, a.workspace_bytes = v.data_ptr(), v.numel() * 4
        elif v is not None:
            setattr(a, n, v.data_ptr())
    return a


def tconv_args(maps, cin, cout, s, slope, **ptr):
    a = _lib.HftTconv()
    a.rows, a.cin, a.cout, a.stride, a.slope = maps.samples, cin, cout, s, slope
    a.seg_lo, a.seg_hi = maps.seg_lo.data_ptr(), maps.seg_hi.data_ptr()
    for n, v in ptr.items():
        if n == "workspace" and v is not None:
            a.workspace, a.workspace_bytes = v.data_ptr(), v.numel() * 4
        elif v is not None:
            setattr(a, n, v.data_ptr())
    return a


def launch_sum(out, terms, scale):
    """out = scale (terms[0] + terms[1] + ..), in that order"""
    arr = (C.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
    _lib.check(_lib.load().fcl_hft_sum(out.data_ptr(), arr, len(terms), scale, out.numel(), ops._stream()))


# on caller-owned buffers (the tests surround them with guard zones)
def launch_stage_forward(plan, maps, stage, c, w, u, units, out):
    """c [rows in, cin] the stage's input, w from pack_weights -> u, units[j][d] = (xt, x') and out = (1 / nk) sum of the blocks' last x' (kept_shapes)"""
    lib, st = _lib.load(), ops._stream()
    ci, co, s, sl = plan.widths[stage], plan.widths[stage + 1], plan.scales[stage], plan.slope
    mo = maps.maps[stage + 1]
    _lib.check(lib.fcl_hft_tconv_fwd(C.byref(tconv_args(maps.maps[stage], ci, co, s, sl, c=c, w=w["tw"], bias=w["tb"], u=u)), st))
    for (k, dils), wb, ub in zip(plan.blocks, w["units"], units):
        x = u
        for dil, wu, (xt, xo) in zip(dils, wb, ub):
            _lib.check(lib.fcl_hft_conv_fwd(C.byref(conv_args(mo, co, co, k, dil, sl, 1, x=x, w=wu["w1"], bias=wu["b1"], y=xt)), st))
            _lib.check(lib.fcl_hft_conv_fwd(C.byref(conv_args(mo, co, co, k, 1, sl, 1, x=xt, w=wu["w2"], bias=wu["b2"], res=x, y=xo)), st))
            x = xo
    launch_sum(out, [ub[-1][1] for ub in units], 1.0 / plan.nk)


def launch_stage_backward(plan, maps, stage, dout, c, w, u, units, dc, dweights, seed, dxt, ping, dxb, du, workspace=None):
    """dout [rows out, cout], the gradient of the stage's output -> dc [rows in, cin] (None: the transposed convolution's input gradient is not launched)
    and dweights = (dwt, dbt, per block per unit (dw1, db1, dw2, db2)) (plan.dweight_shapes; None: no weight-gradient kernel is launched).  Scratch, all
    [rows out, cout]: seed, dxt, ping (two), dxb (one per block), du; workspace: plan.workspace_floats floats (needed with dweights)."""
    lib, st = _lib.load(), ops._stream()
    ci, co, s, sl = plan.widths[stage], plan.widths[stage + 1], plan.scales[stage], plan.slope
    mi, mo = maps.maps[stage], maps.maps[stage + 1]
    launch_sum(seed, [dout], 1.0 / plan.nk)
    for j, ((k, dils), wb, ub) in enumerate(zip(plan.blocks, w["units"], units)):
        g = seed
        for d in range(len(dils) - 1, -1, -1):
            wu, (xt, _), x = wb[d], ub[d], (u if d == 0 else ub[d - 1][1])
            if dweights is not None:
                dw1, db1, dw2, db2 = dweights[2][j][d]
                _lib.check(lib.fcl_hft_conv_dw(C.byref(conv_args(mo, co, co, k, 1, sl, 1, x=xt, g=g, dw=dw2, db=db2, workspace=workspace)), st))
            _lib.check(lib.fcl_hft_conv_dx(C.byref(conv_args(mo, co, co, k, 1, sl, x=g, w=wu["w2_dx"], pre=xt, y=dxt)), st))
            if dweights is not None:
                _lib.check(lib.fcl_hft_conv_dw(C.byref(conv_args(mo, co, co, k, dils[d], sl, 1, x=x, g=dxt, dw=dw1, db=db1, workspace=workspace)), st))
            dx = dxb[j] if d == 0 else ping[d & 1]
            _lib.check(lib.fcl_hft_conv_dx(C.byref(conv_args(mo, co, co, k, dils[d], sl, x=dxt, w=wu["w1_dx"], pre=x, res=g, y=dx)), st))
            g = dx
    launch_sum(du, dxb, 1.0)
    if dweights is not None:
        _lib.check(lib.fcl_hft_tconv_dw(C.byref(tconv_args(mi, ci, co, s, sl, c=c, du=du, dw=dweights[0], db=dweights[1], workspace=workspace)), st))
    if dc is not None:
        _lib.check(lib.fcl_hft_tconv_dx(C.byref(tconv_args(mi, ci, co, s, sl, c=c, w=w["tw_dx"], du=du, dc=dc)), st))


def _new(dev):
    return lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)


class _Stages(torch.autograd.Function):
    """the last stage's output [rows, C] from c0 [frames, channels] (input_conv's output) and the stages' plain parameters (stage_params order, stage by
    stage); backward gives the gradients of all of them that are asked for"""

    @staticmethod
    def forward(ctx, plan, maps, c0, *params):
        dev, per = plan.device, plan.stage_params()
        with torch.cuda.device(dev):
            new = _new(dev)
            c, kept, packed = c0.detach().to(torch.float32).contiguous(), [], []
            for i in range(len(plan.scales)):
                w = pack_weights(plan, i, params[per * i : per * (i + 1)])
                su, sunits, sout = plan.kept_shapes(maps, i)
                u, units, out = new(su), [[(new(a), new(b)) for a, b in blk] for blk in sunits], new(sout)
                launch_stage_forward(plan, maps, i, c, w, u, units, out)
                kept.append((c, u, units))
                packed.append(w)
                c = out
        ctx.plan, ctx.maps, ctx.kept, ctx.packed = plan, maps, kept, packed
        return c

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        plan, maps, dev = ctx.plan, ctx.maps, ctx.plan.device
        need_c, need_w = ctx.needs_input_grad[2], any(ctx.needs_input_grad[3:])
        grads = []
        with torch.cuda.device(dev):
            new = _new(dev)
            work = new(plan.workspace_floats(maps)) if need_w else None
            g = dout.detach().to(torch.float32).contiguous()
            for i in range(len(plan.scales) - 1, -1, -1):
                c, u, units = ctx.kept[i]
                shp = tuple(u.shape)
                dws = None
                if need_w:
                    st, sb, su = plan.dweight_shapes(i)
                    dws = (new(st), new(sb), [[tuple(new(s) for s in unit) for unit in blk] for blk in su])
                dc = new(tuple(c.shape)) if i > 0 or need_c else None
                launch_stage_backward(plan, maps, i, g, c, ctx.packed[i], u, units, dc, dws, new(shp), new(shp), [new(shp), new(shp)],
                                      [new(shp) for _ in plan.blocks], new(shp), work)
                if need_w:
                    grads = unpack_dweights(*dws) + grads
                g = dc
        if not need_w:
            grads = [None] * (len(ctx.needs_input_grad) - 3)
        return (None, None, g) + tuple(grads)


def upsampling_stages(plan, maps, c0, *params):
    """c0 [frames, channels] and the stages' plain parameters -> the last stage's output [frames x hop, channels >> stages]"""
    return _Stages.apply(plan, maps, c0, *params)


class _InputConv(torch.autograd.Function):
    """input_conv on the packed mel rows [frames, in_channels]: the plain-operand convolution, its weight gradient and (if asked) its input gradient"""

    @staticmethod
    def forward(ctx, plan, maps, mel, weight, bias):
        dev, m = plan.device, maps.maps[0]
        with torch.cuda.device(dev):
            mel = mel.detach().to(torch.float32).contiguous()
            wf, wdx = pack_conv(weight)
            y = _new(dev)(m.samples, plan.widths[0])
            a = conv_args(m, plan.in_channels, plan.widths[0], plan.kernel_size, 1, plan.slope, x=mel, w=wf, bias=_f(bias).contiguous(), y=y)
            _lib.check(_lib.load().fcl_hft_conv_fwd(C.byref(a), ops._stream()))
        ctx.plan, ctx.maps, ctx.mel, ctx.wdx = plan, maps, mel, wdx
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        plan, m, dev = ctx.plan, ctx.maps.maps[0], ctx.plan.device
        ci, co, k = plan.in_channels, plan.widths[0], plan.kernel_size
        dmel = dw = db = None
        with torch.cuda.device(dev):
            new, lib, st = _new(dev), _lib.load(), ops._stream()
            dy = dy.detach().to(torch.float32).contiguous()
            if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
                dwk, db = new(k, ci, co), new(co)
                work = new(lib.fcl_hft_workspace_bytes(m.samples, ci, co, k, 1) // 4)
                _lib.check(lib.fcl_hft_conv_dw(C.byref(conv_args(m, ci, co, k, 1, plan.slope, x=ctx.mel, g=dy, dw=dwk, db=db, workspace=work)), st))
                dw = dwk.permute(2, 1, 0).contiguous()
            if ctx.needs_input_grad[2]:
                dmel = new(m.samples, ci)
                _lib.check(lib.fcl_hft_conv_dx(C.byref(conv_args(m, co, ci, k, 1, plan.slope, x=dy, w=ctx.wdx, y=dmel)), st))
        return None, None, dmel, dw, db


def input_conv(plan, maps, mel, weight, bias):
    return _InputConv.apply(plan, maps, mel, weight, bias)


def pack_end(w):
    """torch Conv1d weight (cout, C, k) -> [k, cout, C], the one matrix the output end's three launches read"""
    return _f(w).permute(2, 0, 1).contiguous()


def end_args(maps, cin, cout, k, slope, **ptr):
    a = _lib.HfeEnd()
    a.rows, a.cin, a.cout, a.ksize, a.slope = maps.samples, cin, cout, k, slope
    a.seg_lo, a.seg_hi = maps.seg_lo.data_ptr(), maps.seg_hi.data_ptr()
    for n, v in ptr.items():
        if n == "workspace" and v is not None:
            a.workspace, a.workspace_bytes = v.data_ptr(), v.numel() * 4
        elif v is not None:
            setattr(a, n, v.data_ptr())
    return a


class _OutputEnd(torch.autograd.Function):
    """wav [rows, cout] = tanh(output_conv(LeakyReLU(x))) on the last stage's packed rows x [rows, C]; only wav is kept.  Backward launches the weight
    gradient only if the weight or the bias asks for one, the input gradient only if x does."""

    @staticmethod
    def forward(ctx, plan, maps, x, weight, bias):
        dev, m = plan.device, maps.maps[-1]
        cout, cin, k = (int(v) for v in weight.shape)
        with torch.cuda.device(dev):
            x, w = x.detach().to(torch.float32).contiguous(), pack_end(weight)
            wav = _new(dev)(m.samples, cout)
            a = end_args(m, cin, cout, k, hifigan.OUT_SLOPE, x=x, w=w, bias=_f(bias).contiguous(), wav=wav)
            _lib.check(_lib.load().fcl_hfe_fwd(C.byref(a), ops._stream()))
        ctx.plan, ctx.maps, ctx.x, ctx.w, ctx.wav, ctx.shape = plan, maps, x, w, wav.detach(), (cin, cout, k)
        return wav

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dwav):
        m, dev, (cin, cout, k) = ctx.maps.maps[-1], ctx.plan.device, ctx.shape
        dx = dw = db = None
        with torch.cuda.device(dev):
            new, lib, st = _new(dev), _lib.load(), ops._stream()
            dwav = dwav.detach().to(torch.float32).contiguous()
            if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
                dwk, db = new(k, cout, cin), new(cout)
                work = new(lib.fcl_hfe_workspace_bytes(m.samples, cin, cout, k) // 4)
                a = end_args(m, cin, cout, k, hifigan.OUT_SLOPE, x=ctx.x, wav=ctx.wav, dwav=dwav, dw=dwk, db=db, workspace=work)
                _lib.check(lib.fcl_hfe_dw(C.byref(a), st))
                dw = dwk.permute(1, 2, 0).contiguous()
            if ctx.needs_input_grad[2]:
                dx = new(m.samples, cin)
                _lib.check(lib.fcl_hfe_dx(C.byref(end_args(m, cin, cout, k, hifigan.OUT_SLOPE, x=ctx.x, w=ctx.w, wav=ctx.wav, dwav=dwav, dx=dx)), st))
        return None, None, dx, dw, db


def output_end(plan, maps, x, weight, bias):
    """x [frames x hop, C] (upsampling_stages' result) and output_conv's plain parameters -> the waveform's packed rows [frames x hop, out_channels]"""
    return _OutputEnd.apply(plan, maps, x, weight, bias)


class _TConv(_Conv):
    """a ConvTranspose1d's parameters: weight (cin, cout, k), dim 0 (weight norm's) is the input channel, the bias has cout elements"""

    def __init__(self, shape, weight_norm):
        super().__init__(shape, True, weight_norm)
        self.bias = torch.nn.Parameter(torch.zeros(shape[1]))


class _Seq(torch.nn.Module):
    """index 1 of the reference's Sequential(activation, convolution)"""

    def __init__(self, conv):
        super().__init__()
        self.add_module("1", conv)

    @property
    def conv(self):
        return self._modules["1"]


class _Block(torch.nn.Module):
    def __init__(self, ch, k, n, weight_norm):
        super().__init__()
        self.convs1 = torch.nn.ModuleList([_Seq(_Conv((ch, ch, k), True, weight_norm)) for _ in range(n)])
        self.convs2 = torch.nn.ModuleList([_Seq(_Conv((ch, ch, k), True, weight_norm)) for _ in range(n)])


class TrainableHiFiGANGenerator(_Module):
    """forward(c, lens=None, output_end="torch") -> waveform [B, out_channels, T' hop].  Parameter names and shapes are hifigan.param_spec's (weight_g /
    weight_v under use_weight_norm); weights N(0, 0.01), zero biases, as the reference initialises them."""

    CHECKPOINT_KEY, PLAN = "generator", TrainingPlan

    def __init__(self, in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                 resblock_kernel_sizes=(3, 7, 11), resblock_dilations=((1, 3, 5), (1, 3, 5), (1, 3, 5)), use_additional_convs=True, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params=None, use_weight_norm=True):
        super().__init__()
        act = dict(hifigan.CONFIG["nonlinear_activation_params"] if nonlinear_activation_params is None else nonlinear_activation_params)
        self.config = check_training(hifigan.config(dict(
            in_channels=in_channels, out_channels=out_channels, channels=channels, kernel_size=kernel_size, upsample_scales=upsample_scales,
            upsample_kernel_sizes=upsample_kernel_sizes, resblock_kernel_sizes=resblock_kernel_sizes, resblock_dilations=resblock_dilations,
            use_additional_convs=use_additional_convs, bias=bias, nonlinear_activation=nonlinear_activation, nonlinear_activation_params=act,
            use_weight_norm=bool(use_weight_norm))))
        cfg, wn = self.config, bool(use_weight_norm)
        self.scales, nk = cfg["upsample_scales"], len(cfg["resblock_kernel_sizes"])
        self.hop = 1
        for s in self.scales:
            self.hop *= s
        self.input_conv = _Conv((channels, in_channels, kernel_size), True, wn)
        self.upsamples = torch.nn.ModuleList([_Seq(_TConv((channels >> i, channels >> (i + 1), 2 * s), wn)) for i, s in enumerate(self.scales)])
        self.blocks = torch.nn.ModuleList([_Block(channels >> (i + 1), k, len(cfg["resblock_dilations"][j]), wn)
                                           for i in range(len(self.scales)) for j, k in enumerate(cfg["resblock_kernel_sizes"])])
        self.output_conv = _Seq(_Conv((out_channels, channels >> len(self.scales), kernel_size), True, wn))
        self.nk, self.use_weight_norm = nk, wn
        with torch.no_grad():
            for _, m in self._named_convs():
                w = torch.empty_like(m.folded()).normal_(0.0, 0.01)
                if wn:
                    m.weight_v.copy_(w)
                    m.weight_g.copy_(_norm(w))
                else:
                    m.weight.copy_(w)
        self._reset_cache()

    def cfg(self):
        """the configuration in the form hifigan.HiFiGANPlan takes"""
        return dict(self.config)

    def maps(self, frames):
        """frames per utterance; kept for the next batch of the same lengths"""
        key = tuple(frames)
        if key != self._maps_key:
            self._maps_key, self._maps = key, StageMaps(frames, self.scales, self.plan().device)
        return self._maps

    def stage_parameters(self):
        """the stages' plain (folded) parameters in TrainingPlan.stage_params order"""
        out = []
        for i in range(len(self.scales)):
            t = self.upsamples[i].conv
            out += [t.folded(), t.bias]
            for j in range(self.nk):
                blk = self.blocks[i * self.nk + j]
                for c1, c2 in zip(blk.convs1, blk.convs2):
                    out += [c1.conv.folded(), c1.conv.bias, c2.conv.folded(), c2.conv.bias]
        return out

    def forward(self, c, lens=None, output_end="torch"):
        """c [B, in_channels, T']; lens (frames per utterance): the rows past lens[b] are padding, come out as zero and get exactly zero gradient, and
        every utterance is computed as if it were alone.  output_end: "torch" runs LeakyReLU, output_conv and tanh as torch operations on the padded
        batch, "hip" as the hfe_* launches on the packed rows (only the [rows, out_channels] waveform is unpacked)."""
        if output_end not in OUTPUT_ENDS:
            raise ValueError("fcl-taco2_amd: HiFi-GAN generator: output_end=%r is not one of %s" % (output_end, ", ".join(repr(v) for v in OUTPUT_ENDS)))
        plan = self.plan()
        c = torch.as_tensor(c).to(device=plan.device, dtype=torch.float32)
        if c.dim() != 3 or c.shape[1] != self.config["in_channels"]:
            raise ValueError("fcl-taco2_amd: HiFi-GAN generator: c [B, %d, T'] expected, got %r" % (self.config["in_channels"], tuple(c.shape)))
        B, T = int(c.shape[0]), int(c.shape[2])
        rows = c.transpose(1, 2).reshape(B * T, -1)
        if lens is None:
            maps = self.maps([T] * B)
        else:
            lens = [int(n) for n in lens]
            if len(lens) != B or min(lens) < 1 or max(lens) > T:
                raise ValueError("fcl-taco2_amd: HiFi-GAN generator: lens %r (frames) do not fit %d frames" % (lens, T))
            maps = self.maps(lens)
            rows = rows[maps.rows(T, 1)]
        c0 = input_conv(plan, maps, rows.contiguous(), self.input_conv.folded(), self.input_conv.bias)
        x = upsampling_stages(plan, maps, c0, *self.stage_parameters())
        oc = self.output_conv.conv
        if output_end == "hip":
            y = _OutputEnd.apply(plan, maps, x, oc.folded(), oc.bias)
            if lens is not None:
                y = torch.zeros(B * T * self.hop, y.shape[1], device=y.device, dtype=y.dtype).index_copy(0, maps.rows(T, self.hop), y)
            return y.reshape(B, T * self.hop, -1).transpose(1, 2).contiguous()
        if lens is not None:
            x = torch.zeros(B * T * self.hop, x.shape[1], device=x.device, dtype=x.dtype).index_copy(0, maps.rows(T, self.hop), x)
        x = x.reshape(B, T * self.hop, -1).transpose(1, 2)
        y = torch.tanh(F.conv1d(F.leaky_relu(x, hifigan.OUT_SLOPE), oc.folded(), oc.bias, padding=(self.config["kernel_size"] - 1) // 2))
        if lens is not None:
            y = y * (torch.arange(T * self.hop, device=y.device).unsqueeze(0) < torch.tensor(lens, device=y.device).unsqueeze(1) * self.hop).unsqueeze(1)
        return y
