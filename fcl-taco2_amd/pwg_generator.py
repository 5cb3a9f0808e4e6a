"""The Parallel WaveGAN generator in its training form: the residual stack forward (activations kept) and backward on the HIP path (the pwt_* kernels of
csrc/pwg_train.hip), under an nn.Module with the parallel_wavegan package's constructor arguments and parameter names.

    gen = TrainableParallelWaveGANGenerator().to("cuda:0")
    fake = gen(z, c)                     # z [B, 1, T] noise, c [B, aux, T / hop + 2 ctx] features (replicate-padded) -> [B, 1, T]
    loss(fake).backward()                # the 30 residual blocks and the layers around them run backward in HIP kernels; torch folds weight norm
    vocoder.PWGPlan(gen.state_dict(), "cuda:0")   # the inference generator takes the trained weights as they are

The block's contract is stated in include/fcl_hip.h "Parallel WaveGAN generator, training form" and restated in float64 numpy in tests/pwgt_ref.py; the
forward pass is oracle/pwg_oracle.generator_forward.  Activations are float32, channel-last [samples, C], the batch packed with the utterances back to
back; per block the input x_l [samples, R] and the gate activations ab_l = (tanh | sigmoid) [samples, 2 R] are kept.  One arithmetic mode (exact fp32).
The generator's two ends -- the upsampling network and first_conv in front of the stack, the sqrt(1 / layers) scale and the two last ReLU + 1x1 layers
behind it -- run on the HIP path too (the pwe_* kernels of csrc/pwg_ends.hip; restated in tests/pwge_ref.py); forward(..., ends="torch")
keeps them as torch operations under autograd.  Weight norm is folded in torch in front of the functions.  No CPU fallback."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

from . import _lib, ops
from .pwg_common import Maps, _Conv, _Module  # noqa: F401 (Maps: the packed batch's seg_lo / seg_hi, used through this module too)

KERNEL_SIZES = (3, 5)
BLOCK_PARAMS = ("conv.weight", "conv.bias", "conv1x1_aux.weight", "conv1x1_out.weight", "conv1x1_out.bias", "conv1x1_skip.weight", "conv1x1_skip.bias")
FWD_KERNELS = ("pwt_gate_kernel", "pwt_out_kernel")
DZ_KERNEL, DX_KERNEL, DC_KERNEL = "pwt_dz_kernel", "pwt_dx_kernel", "pwt_dc_kernel"
DW_KERNELS = ("pwt_dw_kernel<gate>", "pwt_dw_kernel<out>", "pwt_dw_reduce_kernel")
DEFAULT_UPSAMPLE = {"upsample_scales": [4, 4, 4, 4]}
IN_FWD_KERNELS = ("pwe_convin_kernel", "pwe_stage_kernel", "pwe_first_kernel")
IN_DW_KERNELS = ("pwe_outer_kernel", "pwe_dh_kernel", "pwe_dwin_kernel", "pwe_reduce_kernel")
IN_DU_KERNEL, IN_DC_KERNEL, IN_DZ_KERNEL = "pwe_stage_bwd_kernel", "pwe_dc_kernel", "pwe_first_dz_kernel"
OUT_FWD_KERNEL, OUT_DX_KERNELS = "pwe_out_kernel", ("pwe_dy1_kernel", "pwe_ds_kernel")
OUT_DW_KERNELS = ("pwe_dw_kernel<last>", "pwe_outer_kernel", "pwe_reduce_kernel")
MAX_SCALES, MAX_SCALE, MAX_CONTEXT = 6, 16, 8


def check_configuration(in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128, skip_channels=64,
                        aux_channels=80, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True, use_causal_conv=False,
                        upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork", upsample_params=None):
    """-> the dilation of every block; anything the kernels do not cover is refused by the argument's name"""
    bad = lambda name, got, want: ValueError("fcl-taco2_amd: PWG generator: %s=%r is not supported on the HIP path (%s)" % (name, got, want))
    if in_channels != 1:
        raise bad("in_channels", in_channels, "1")
    if out_channels != 1:
        raise bad("out_channels", out_channels, "1")
    if kernel_size not in KERNEL_SIZES:
        raise bad("kernel_size", kernel_size, "3 or 5")
    if not (isinstance(layers, int) and 1 <= layers <= 60):
        raise bad("layers", layers, "1 to 60")
    if not (isinstance(stacks, int) and stacks >= 1 and layers % stacks == 0):
        raise bad("stacks", stacks, "a divisor of layers")
    if not (isinstance(residual_channels, int) and 16 <= residual_channels <= 64 and residual_channels % 16 == 0):
        raise bad("residual_channels", residual_channels, "a multiple of 16 from 16 to 64")
    if gate_channels != 2 * residual_channels:
        raise bad("gate_channels", gate_channels, "2 x residual_channels")
    if skip_channels != residual_channels:
        raise bad("skip_channels", skip_channels, "residual_channels")
    if not (isinstance(aux_channels, int) and 16 <= aux_channels <= 128 and aux_channels % 16 == 0):
        raise bad("aux_channels", aux_channels, "a multiple of 16 from 16 to 128")
    if not (isinstance(aux_context_window, int) and aux_context_window >= 0):
        raise bad("aux_context_window", aux_context_window, "an integer >= 0")
    if float(dropout) != 0.0:
        raise bad("dropout", dropout, "0")
    if bias is not True:
        raise bad("bias", bias, "True")
    if use_weight_norm not in (True, False):
        raise bad("use_weight_norm", use_weight_norm, "True or False")
    if use_causal_conv:
        raise bad("use_causal_conv", use_causal_conv, "False")
    if not upsample_conditional_features:
        raise bad("upsample_conditional_features", upsample_conditional_features, "True")
    if upsample_net != "ConvInUpsampleNetwork":
        raise bad("upsample_net", upsample_net, "ConvInUpsampleNetwork")
    params = dict(DEFAULT_UPSAMPLE if upsample_params is None else upsample_params)
    scales = params.pop("upsample_scales", None)
    if params or not scales or any(not (isinstance(s, int) and s >= 1) for s in scales):
        raise bad("upsample_params", upsample_params, "upsample_scales: a list of positive integers, nothing else")
    per = layers // stacks
    if per > 31:
        raise bad("stacks", stacks, "layers / stacks at most 31: a dilation below 2^31")
    return [2 ** (l % per) for l in range(layers)]


def check_ends(upsample_scales, aux_context_window):
    """what the HIP ends cover beyond check_configuration: 1 to 6 scales of 2 to 16 each, a context window of 0 to 8"""
    bad = lambda name, got, want: ValueError("fcl-taco2_amd: PWG generator: %s=%r is not supported on the HIP path (%s)" % (name, got, want))
    scales = list(upsample_scales)
    if not 1 <= len(scales) <= MAX_SCALES or any(not (isinstance(s, int) and 2 <= s <= MAX_SCALE) for s in scales):
        raise bad("upsample_scales", upsample_scales, "1 to %d scales, each 2 to %d" % (MAX_SCALES, MAX_SCALE))
    if not (isinstance(aux_context_window, int) and 0 <= aux_context_window <= MAX_CONTEXT):
        raise bad("aux_context_window", aux_context_window, "0 to %d" % MAX_CONTEXT)


class FrameMaps(Maps):
    """Maps of a batch given in frames per utterance: the sample tables at `hop` samples per frame, and frame_off [n_utt + 1] int32 on the device"""

    def __init__(self, frames, hop, device):
        self.frames, self.hop = [int(f) for f in frames], int(hop)
        super().__init__([f * self.hop for f in self.frames], device)
        self.n_frames = sum(self.frames)
        off = [0]
        for f in self.frames:
            off.append(off[-1] + f)
        self.frame_off = torch.tensor(off, dtype=torch.int32).to(device)
        self._rows = {}

    def rows(self, T, ctx):
        """(z_rows, c_rows) int64 on the device: where the pack's samples sit in a padded batch's [B T] samples, and the pack's conditioning rows in its
        [B (T / hop + 2 ctx)] rows, in the pack's order (built once per padded length)"""
        if (T, ctx) not in self._rows:
            ln = torch.tensor(self.frames).unsqueeze(1)
            zm = torch.arange(T).unsqueeze(0) < ln * self.hop
            cm = torch.arange(T // self.hop + 2 * ctx).unsqueeze(0) < ln + 2 * ctx
            self._rows[(T, ctx)] = tuple(torch.nonzero(m.reshape(-1))[:, 0].to(self.seg_lo.device) for m in (zm, cm))
        return self._rows[(T, ctx)]


class GeneratorPlan(object):
    """Per-block geometry (the dilations) and the sizes of what a pass over n samples needs"""

    def __init__(self, device="cuda:0", **config):
        self.dilations = check_configuration(**config)
        cfg = dict(kernel_size=3, layers=30, stacks=3, residual_channels=64, aux_channels=80)
        cfg.update({k: v for k, v in config.items() if k in cfg})
        self.kernel_size, self.layers, self.stacks, self.R, self.A = (cfg[k] for k in ("kernel_size", "layers", "stacks", "residual_channels", "aux_channels"))
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: GeneratorPlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)
        self.receptive_field = 1 + (self.kernel_size - 1) * sum(self.dilations)
        # the ends (§6o); check_ends refuses what they do not cover where they are used, so that a plan of such a geometry still serves the stack
        self.scales = tuple((config.get("upsample_params") or DEFAULT_UPSAMPLE)["upsample_scales"])
        self.ctx, self.hop, self.sigma = config.get("aux_context_window", 2), int(math.prod(self.scales)), math.sqrt(1.0 / self.layers)

    def stage_rows(self, frames):
        """rows of u_0 .. u_{n - 1}, the stage inputs the input side keeps"""
        rows, out = frames, []
        for s in self.scales:
            out.append(rows)
            rows *= s
        return out

    def ends_workspace_floats(self, maps):
        check_ends(self.scales, self.ctx)
        return _lib.load().fcl_pwe_workspace_bytes(C.byref(_ends_args(self, maps))) // 4

    def kept_shapes(self, n):
        """what the forward pass keeps: x_0 .. x_layers [n, R] (x_layers, the last block's output, is read by nobody) and ab_0 .. ab_{layers - 1} [n, 2 R]"""
        return [(n, self.R)] * (self.layers + 1), [(n, 2 * self.R)] * self.layers

    def kept_bytes(self, n):
        return 4 * n * 3 * self.R * self.layers

    def workspace_floats(self, n):
        """the partials of a block's larger weight gradient"""
        return _lib.load().fcl_pwt_dw_workspace_bytes(n, self.R, self.A, self.kernel_size) // 4

    def dweight_shapes(self):
        """per block (dw_gate [k R + A, 2 R], db_gate [2 R], dw_out [R, 2 R], db_out [2 R]) in the kernels' layout"""
        R = self.R
        return ((self.kernel_size * R + self.A, 2 * R), (2 * R,), (R, 2 * R), (2 * R,))


def pack_weights(blocks):
    """per block the seven torch parameters in BLOCK_PARAMS order -> dict of the kernels' forms (include/fcl_hip.h), contiguous float32.  The backward
    forms are permutations of the forward ones; nothing here is differentiated."""
    out = []
    for conv_w, conv_b, aux_w, out_w, out_b, skip_w, skip_b in blocks:
        f = lambda v: v.detach().to(torch.float32)
        conv_w, aux_w, out_w, skip_w = f(conv_w), f(aux_w)[:, :, 0], f(out_w)[:, :, 0], f(skip_w)[:, :, 0]
        G, R, k = conv_w.shape
        out.append(dict(
            w_gate=torch.cat([conv_w.permute(2, 1, 0).reshape(k * R, G), aux_w.t()]).contiguous(), b_gate=f(conv_b).contiguous(),
            w_out=torch.cat([out_w.t(), skip_w.t()], dim=1).contiguous(), b_out=torch.cat([f(out_b), f(skip_b)]).contiguous(),
            w_dz=torch.cat([out_w, skip_w]).contiguous(), w_dx=conv_w.flip(2).permute(2, 0, 1).contiguous(), w_dc=aux_w.contiguous()))
    return out


def unpack_dweights(plan, dw_gate, db_gate, dw_out, db_out):
    """the kernels' gradient forms of one block -> torch's, in BLOCK_PARAMS order"""
    R, k = plan.R, plan.kernel_size
    return (dw_gate[: k * R].reshape(k, R, 2 * R).permute(2, 1, 0).contiguous(), db_gate, dw_gate[k * R :].t().unsqueeze(2).contiguous(),
            dw_out[:, :R].t().unsqueeze(2).contiguous(), db_out[:R].contiguous(), dw_out[:, R:].t().unsqueeze(2).contiguous(), db_out[R:].contiguous())


def _args(plan, maps, block, first=False, last=False, **ptr):
    a = _lib.PwtBlock()
    a.samples, a.residual, a.aux, a.ksize, a.dilation = maps.samples, plan.R, plan.A, plan.kernel_size, plan.dilations[block]
    a.first, a.last = int(first), int(last)
    a.seg_lo, a.seg_hi = maps.seg_lo.data_ptr(), maps.seg_hi.data_ptr()
    for k, v in ptr.items():
        if v is not None:
            setattr(a, k, v.data_ptr())
    return a


# on caller-owned buffers (the tests surround them with guard zones)
def launch_forward(plan, maps, c, weights, xs, abs_, skips, z_outs=None):
    """xs[0] [samples, R] the stack's input, c [samples, A], weights from pack_weights -> xs[1 ..], abs_[l] (plan.kept_shapes) and skips [samples, R],
    the un-scaled skip sum (written by block 0, added to by the others).  z_outs (tests): per block a [samples, 2 R] buffer for the pre-activations."""
    lib, st = _lib.load(), ops._stream()
    for l, w in enumerate(weights):
        a = _args(plan, maps, l, first=l == 0, x=xs[l], c=c, w_gate=w["w_gate"], b_gate=w["b_gate"], w_out=w["w_out"], b_out=w["b_out"], ab=abs_[l],
                  x_out=xs[l + 1], skips=skips, z_out=None if z_outs is None else z_outs[l])
        _lib.check(lib.fcl_pwt_block_fwd(C.byref(a), st))


def launch_backward(plan, maps, ds, c, weights, xs, abs_, dx0, dc, dweights, grads, dz, workspace=None):
    """ds [samples, R], the gradient of the un-scaled skip sum -> dx0 [samples, R] (None: block 0's conv-backward is not launched), dc [samples, A]
    (None: no aux-backward is launched; written by the last block, added to by the others) and dweights = per block (dw_gate, db_gate, dw_out, db_out)
    (plan.dweight_shapes; None: no weight-gradient kernel is launched).  grads: two [samples, R] buffers, dz: one [samples, 2 R] buffer, workspace:
    plan.workspace_floats(samples) floats (needed with dweights)."""
    lib, st = _lib.load(), ops._stream()
    g = None
    for l in range(plan.layers - 1, -1, -1):
        w, last = weights[l], l == plan.layers - 1
        out = grads[l & 1] if l > 0 else dx0
        a = _args(plan, maps, l, last=last, x=xs[l], c=c, ab=abs_[l], dxo=g, ds=ds, w_dz=w["w_dz"], w_dx=w["w_dx"], w_dc=w["w_dc"], dz=dz, dx=out, dc=dc)
        _lib.check(lib.fcl_pwt_block_dx(C.byref(a), st))
        if dweights is not None:
            a.dw_gate, a.db_gate, a.dw_out, a.db_out = (b.data_ptr() for b in dweights[l])
            a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
            _lib.check(lib.fcl_pwt_block_dw(C.byref(a), st))
        g = out


class _Function(torch.autograd.Function):
    """the un-scaled skip sum [samples, R] of the residual stack on x_0 [samples, R], c [samples, A] and the blocks' plain weights (BLOCK_PARAMS order,
    block by block); backward gives the gradients of all of them that are asked for"""

    @staticmethod
    def forward(ctx, plan, maps, x0, c, *params):
        dev, n = plan.device, maps.samples
        blocks = [params[7 * l : 7 * l + 7] for l in range(plan.layers)]
        with torch.cuda.device(dev):
            new = lambda s: torch.empty(s, device=dev, dtype=torch.float32)
            packed = pack_weights(blocks)
            sx, sab = plan.kept_shapes(n)
            xs, abs_ = [x0.detach().to(torch.float32).contiguous()] + [new(s) for s in sx[1:]], [new(s) for s in sab]
            c = c.detach().to(torch.float32).contiguous()
            skips = new((n, plan.R))
            launch_forward(plan, maps, c, packed, xs, abs_, skips)
        ctx.plan, ctx.maps, ctx.packed, ctx.xs, ctx.abs, ctx.c = plan, maps, packed, xs[:-1], abs_, c
        return skips

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ds):
        plan, maps, dev, n = ctx.plan, ctx.maps, ctx.plan.device, ctx.maps.samples
        need_x, need_c, need_w = ctx.needs_input_grad[2], ctx.needs_input_grad[3], any(ctx.needs_input_grad[4:])
        with torch.cuda.device(dev):
            new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
            dx0, dc = new(n, plan.R) if need_x else None, new(n, plan.A) if need_c else None
            dweights = [tuple(new(s) for s in plan.dweight_shapes()) for _ in range(plan.layers)] if need_w else None
            launch_backward(plan, maps, ds.detach().to(torch.float32).contiguous(), ctx.c, ctx.packed, ctx.xs, ctx.abs, dx0, dc, dweights,
                            grads=[new(n, plan.R), new(n, plan.R)], dz=new(n, 2 * plan.R), workspace=new(plan.workspace_floats(n)) if need_w else None)
        out = [None, None, dx0, dc]
        if need_w:
            for dw in dweights:
                out += unpack_dweights(plan, *dw)
        else:
            out += [None] * (len(ctx.needs_input_grad) - 4)
        return tuple(out)


def residual_stack(plan, maps, x0, c, blocks):
    """blocks: per block the seven plain parameters in BLOCK_PARAMS order -> the un-scaled skip sum [samples, R]"""
    return _Function.apply(plan, maps, x0, c, *[p for b in blocks for p in b])


def pack_in_weights(win, hs, w0, b0):
    """the input side's plain torch parameters (conv_in, the stage filters, first_conv) -> the kernels' forms (include/fcl_hip.h)"""
    f = lambda v: v.detach().to(torch.float32)
    return dict(w_in=f(win).permute(2, 1, 0).reshape(-1, win.shape[0]).contiguous(), h=[f(h).reshape(-1).contiguous() for h in hs],
                w0=f(w0).reshape(-1).contiguous(), b0=f(b0).contiguous())


def pack_out_weights(w1, b1, w3, b3):
    """last_conv_layers 1 and 3 -> the kernels' forms: W1 in both orientations, the last layer as a vector and a one-element bias"""
    f = lambda v: v.detach().to(torch.float32)
    return dict(w1=f(w1)[:, :, 0].t().contiguous(), w1t=f(w1)[:, :, 0].contiguous(), b1=f(b1).contiguous(), w3=f(w3).reshape(-1).contiguous(),
                b3=f(b3).reshape(1).contiguous())


def _ends_args(plan, maps, **ptr):
    a = _lib.PweEnds()
    a.samples, a.frames, a.n_utt = maps.samples, maps.n_frames, maps.n_utt
    a.residual, a.aux, a.ctx, a.n_scales, a.sigma = plan.R, plan.A, plan.ctx, len(plan.scales), plan.sigma
    for i, s in enumerate(plan.scales):
        a.scales[i] = s
    a.seg_lo, a.seg_hi, a.frame_off = maps.seg_lo.data_ptr(), maps.seg_hi.data_ptr(), maps.frame_off.data_ptr()
    for k, v in ptr.items():
        if v is None:
            continue
        if isinstance(v, (list, tuple)):
            for i, b in enumerate(v):
                getattr(a, k)[i] = b.data_ptr()
        elif k == "workspace":
            a.workspace, a.workspace_bytes = v.data_ptr(), v.numel() * 4
        else:
            setattr(a, k, v.data_ptr())
    return a


# on caller-owned buffers, as launch_forward / launch_backward
def launch_in_forward(plan, maps, z, c, w, us, cu, x0):
    """z [samples], c [frames + 2 ctx n_utt, A], w from pack_in_weights -> us (plan.stage_rows: u_i [rows_i, A], kept), cu [samples, A], x0 [samples, R]"""
    check_ends(plan.scales, plan.ctx)
    a = _ends_args(plan, maps, z=z, c=c, w_in=w["w_in"], h=w["h"], w0=w["w0"], b0=w["b0"], u=us, cu=cu, x0=x0)
    _lib.check(_lib.load().fcl_pwe_in_fwd(C.byref(a), ops._stream()))


def launch_in_backward(plan, maps, dcu, dx0, z, c, w, us, dweights, dc, dz, workspace):
    """dcu [samples, A], dx0 [samples, R] -> dweights = (dw_in [(2 ctx + 1) A, A], [dh_i], dw0 [R], db0 [R]) (None: no weight-gradient kernel is
    launched), dc (None: not computed), dz [samples] (None: not computed); workspace: plan.ends_workspace_floats floats (needed with dweights or dc)"""
    check_ends(plan.scales, plan.ctx)
    a = _ends_args(plan, maps, dcu=dcu, dx0=dx0, z=z, c=c, w_in=w["w_in"], h=w["h"], w0=w["w0"], u=us, dc=dc, dz=dz, workspace=workspace)
    if dweights is not None:
        a.dw_in, a.dw0, a.db0 = dweights[0].data_ptr(), dweights[2].data_ptr(), dweights[3].data_ptr()
        for i, b in enumerate(dweights[1]):
            a.dh[i] = b.data_ptr()
    _lib.check(_lib.load().fcl_pwe_in_bwd(C.byref(a), ops._stream()))


def launch_out_forward(plan, maps, skips, w, y1, wav):
    """skips [samples, R] -> y1 [samples, R] (kept), wav [samples]"""
    a = _ends_args(plan, maps, skips=skips, w1=w["w1"], b1=w["b1"], w3=w["w3"], b3=w["b3"], y1=y1, wav=wav)
    _lib.check(_lib.load().fcl_pwe_out_fwd(C.byref(a), ops._stream()))


def launch_out_backward(plan, maps, dwav, skips, y1, w, dy1, ds, dweights, workspace):
    """dwav [samples] -> ds [samples, R] (dy1 [samples, R] is scratch) and dweights = (dw1 [R, R] (row: input channel), db1 [R], dw3 [R], db3 [1])
    (None: no weight-gradient kernel is launched; workspace is needed with them)"""
    a = _ends_args(plan, maps, dwav=dwav, skips=skips, y1=y1, w1t=w["w1t"], w3=w["w3"], dy1=dy1, ds=ds, workspace=workspace)
    if dweights is not None:
        a.dw1, a.db1, a.dw3, a.db3 = (b.data_ptr() for b in dweights)
    _lib.check(_lib.load().fcl_pwe_out_bwd(C.byref(a), ops._stream()))


def _new(dev):
    return lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)


class _InputEnd(torch.autograd.Function):
    """(cu [samples, A], x0 [samples, R]) from the packed noise z [samples], the packed conditioning c [frames + 2 ctx n_utt, A] and the plain weights
    conv_in, the stage filters, first_conv weight and bias"""

    @staticmethod
    def forward(ctx, plan, maps, z, c, win, w0, b0, *hs):
        dev, n = plan.device, maps.samples
        with torch.cuda.device(dev):
            new = _new(dev)
            w = pack_in_weights(win, hs, w0, b0)
            z, c = z.detach().to(torch.float32).contiguous(), c.detach().to(torch.float32).contiguous()
            us, cu, x0 = [new(r, plan.A) for r in plan.stage_rows(maps.n_frames)], new(n, plan.A), new(n, plan.R)
            launch_in_forward(plan, maps, z, c, w, us, cu, x0)
        ctx.plan, ctx.maps, ctx.w, ctx.z, ctx.c, ctx.us = plan, maps, w, z, c, us
        return cu, x0

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dcu, dx0):
        plan, maps, dev, n = ctx.plan, ctx.maps, ctx.plan.device, ctx.maps.samples
        need_z, need_c, need_w = ctx.needs_input_grad[2], ctx.needs_input_grad[3], any(ctx.needs_input_grad[4:])
        with torch.cuda.device(dev):
            new = _new(dev)
            K = (2 * plan.ctx + 1) * plan.A
            dws = (new(K, plan.A), [new(2 * s + 1) for s in plan.scales], new(plan.R), new(plan.R)) if need_w else None
            dc, dz = new(tuple(ctx.c.shape)) if need_c else None, new(n) if need_z else None
            work = new(plan.ends_workspace_floats(maps)) if need_w or need_c else None
            launch_in_backward(plan, maps, dcu.detach().to(torch.float32).contiguous(), dx0.detach().to(torch.float32).contiguous(), ctx.z, ctx.c, ctx.w,
                               ctx.us, dws, dc, dz, work)
        if not need_w:
            return (None, None, dz, dc) + (None,) * (len(ctx.needs_input_grad) - 4)
        A, R = plan.A, plan.R
        return (None, None, dz, dc, dws[0].reshape(2 * plan.ctx + 1, A, A).permute(2, 1, 0).contiguous(), dws[2].reshape(R, 1, 1), dws[3]) + tuple(
            h.reshape(1, 1, 1, -1) for h in dws[1])


class _OutputEnd(torch.autograd.Function):
    """the waveform [samples] from the stack's un-scaled skip sum [samples, R] and the plain weights of last_conv_layers 1 and 3"""

    @staticmethod
    def forward(ctx, plan, maps, skips, w1, b1, w3, b3):
        dev, n = plan.device, maps.samples
        with torch.cuda.device(dev):
            new = _new(dev)
            w = pack_out_weights(w1, b1, w3, b3)
            skips = skips.detach().to(torch.float32).contiguous()
            y1, wav = new(n, plan.R), new(n)
            launch_out_forward(plan, maps, skips, w, y1, wav)
        ctx.plan, ctx.maps, ctx.w, ctx.skips, ctx.y1 = plan, maps, w, skips, y1
        return wav

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dwav):
        plan, maps, dev, n, R = ctx.plan, ctx.maps, ctx.plan.device, ctx.maps.samples, ctx.plan.R
        need_w = any(ctx.needs_input_grad[3:])
        with torch.cuda.device(dev):
            new = _new(dev)
            dws = (new(R, R), new(R), new(R), new(1)) if need_w else None
            ds = new(n, R)
            launch_out_backward(plan, maps, dwav.detach().to(torch.float32).contiguous(), ctx.skips, ctx.y1, ctx.w, new(n, R), ds, dws,
                                new(plan.ends_workspace_floats(maps)) if need_w else None)
        if not need_w:
            return None, None, ds, None, None, None, None
        return None, None, ds, dws[0].t().unsqueeze(2).contiguous(), dws[1], dws[2].reshape(1, R, 1), dws[3]


def input_end(plan, maps, z, c, win, hs, w0, b0):
    """-> (cu [samples, A], x0 [samples, R]); maps: FrameMaps"""
    return _InputEnd.apply(plan, maps, z, c, win, w0, b0, *hs)


def output_end(plan, maps, skips, w1, b1, w3, b3):
    """-> the waveform [samples]"""
    return _OutputEnd.apply(plan, maps, skips, w1, b1, w3, b3)


class _Holder(torch.nn.Module):  # an index of the reference's Sequential / ModuleList that holds no parameter (Stretch2d, ReLU), or a plain container
    pass


class _Block(torch.nn.Module):
    def __init__(self, R, A, k, weight_norm):
        super().__init__()
        self.conv = _Conv((2 * R, R, k), True, weight_norm)
        self.conv1x1_aux = _Conv((2 * R, A, 1), False, weight_norm)
        self.conv1x1_out = _Conv((R, R, 1), True, weight_norm)
        self.conv1x1_skip = _Conv((R, R, 1), True, weight_norm)

    def plain(self):
        """BLOCK_PARAMS order"""
        return (self.conv.folded(), self.conv.bias, self.conv1x1_aux.folded(), self.conv1x1_out.folded(), self.conv1x1_out.bias,
                self.conv1x1_skip.folded(), self.conv1x1_skip.bias)


class TrainableParallelWaveGANGenerator(_Module):
    """forward(z, c, lens=None, ends="hip") -> waveform [B, 1, T].  Parameter names and shapes are vocoder.param_spec's (weight_g / weight_v under use_weight_norm);
    Kaiming-normal weights, zero biases, smoothing filters 1 / (2 s + 1), as the reference initialises them."""

    CHECKPOINT_KEY, PLAN = "generator", GeneratorPlan

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128, skip_channels=64,
                 aux_channels=80, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True, use_causal_conv=False,
                 upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork", upsample_params=None):
        super().__init__()
        self.config = dict(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, layers=layers, stacks=stacks,
                           residual_channels=residual_channels, gate_channels=gate_channels, skip_channels=skip_channels, aux_channels=aux_channels,
                           aux_context_window=aux_context_window, dropout=dropout, bias=bias, use_weight_norm=use_weight_norm,
                           use_causal_conv=use_causal_conv, upsample_conditional_features=upsample_conditional_features, upsample_net=upsample_net,
                           upsample_params=dict(DEFAULT_UPSAMPLE if upsample_params is None else upsample_params))
        check_configuration(**self.config)
        R, A, wn = residual_channels, aux_channels, bool(use_weight_norm)
        self.scales = tuple(int(s) for s in self.config["upsample_params"]["upsample_scales"])
        self.hop, self.ctx = int(math.prod(self.scales)), int(aux_context_window)
        self.first_conv = _Conv((R, 1, 1), True, wn)
        self.upsample_net = _Holder()
        self.upsample_net.conv_in = _Conv((A, A, 2 * self.ctx + 1), False, wn)
        self.upsample_net.upsample = _Holder()
        ups = []
        for s in self.scales:
            ups += [_Holder(), _Conv((1, 1, 1, 2 * s + 1), False, wn, init=1.0 / (2 * s + 1))]
        self.upsample_net.upsample.up_layers = torch.nn.ModuleList(ups)
        self.conv_layers = torch.nn.ModuleList([_Block(R, A, kernel_size, wn) for _ in range(layers)])
        self.last_conv_layers = torch.nn.ModuleList([_Holder(), _Conv((R, R, 1), True, wn), _Holder(), _Conv((1, R, 1), True, wn)])
        self.use_weight_norm = wn
        self._reset_cache()

    def cfg(self):
        """the configuration in the form vocoder.PWGPlan takes"""
        c = self.config
        return dict(layers=c["layers"], stacks=c["stacks"], residual_channels=c["residual_channels"], gate_channels=c["gate_channels"],
                    skip_channels=c["skip_channels"], aux_channels=c["aux_channels"], aux_context_window=c["aux_context_window"],
                    kernel_size=c["kernel_size"], upsample_scales=self.scales)

    convs = _Module._named_convs

    def upsample(self, c):
        """ConvInUpsampleNetwork: c [B, A, T' + 2 ctx] -> [B, A, T' hop] (torch operations)"""
        c = F.conv1d(c, self.upsample_net.conv_in.folded()).unsqueeze(1)
        for i, s in enumerate(self.scales):
            c = F.interpolate(c, scale_factor=(1, s), mode="nearest")
            c = F.conv2d(c, self.upsample_net.upsample.up_layers[2 * i + 1].folded(), padding=(0, s))
        return c.squeeze(1)

    def maps(self, lens):
        """lens in samples (multiples of the hop); kept for the next batch of the same lengths"""
        key = tuple(lens)
        if key != self._maps_key:
            self._maps_key, self._maps = key, FrameMaps([n // self.hop for n in lens], self.hop, self.plan().device)
        return self._maps

    def forward(self, z, c, lens=None, ends="hip"):
        """z [B, 1, T], c [B, A, T / hop + 2 ctx]; lens (frames per utterance): the rows past lens[b] * hop are padding, come out as zero and get exactly
        zero gradient, and every utterance is computed as if it were alone.  ends: "hip", the ends in the pwe_* kernels, or "torch", as torch operations
        (the reference of the tests and the other leg of the timing)"""
        if ends not in ("hip", "torch"):
            raise ValueError("fcl-taco2_amd: PWG generator: ends=%r is not \"hip\" or \"torch\"" % (ends,))
        dev = self.plan().device
        z, c = torch.as_tensor(z).to(device=dev, dtype=torch.float32), torch.as_tensor(c).to(device=dev, dtype=torch.float32)
        if z.dim() != 3 or z.shape[1] != 1 or c.dim() != 3 or c.shape[1] != self.config["aux_channels"] or c.shape[0] != z.shape[0]:
            raise ValueError("fcl-taco2_amd: PWG generator: z [B, 1, T] and c [B, %d, T / hop + 2 ctx] expected, got %r and %r"
                             % (self.config["aux_channels"], tuple(z.shape), tuple(c.shape)))
        B, T = int(z.shape[0]), int(z.shape[2])
        if (int(c.shape[2]) - 2 * self.ctx) * self.hop != T:
            raise ValueError("fcl-taco2_amd: PWG generator: %d frames (+ 2 x %d of context) at hop %d do not make %d samples"
                             % (int(c.shape[2]) - 2 * self.ctx, self.ctx, self.hop, T))
        if ends == "hip":
            return self._forward_hip(z, c, lens, B, T)
        x = F.conv1d(z, self.first_conv.folded(), self.first_conv.bias).transpose(1, 2)  # [B, T, R]
        if lens is None:
            n_of = [T] * B
            x0, cu = x.reshape(B * T, -1), self.upsample(c).transpose(1, 2).reshape(B * T, -1)
        else:
            lens = [int(n) for n in lens]
            if len(lens) != B or min(lens) < 1 or max(lens) * self.hop > T:
                raise ValueError("fcl-taco2_amd: PWG generator: lens %r (frames) do not fit %d samples at hop %d" % (lens, T, self.hop))
            n_of = [n * self.hop for n in lens]
            x0 = torch.cat([x[b, :n] for b, n in enumerate(n_of)])
            cu = torch.cat([self.upsample(c[b : b + 1, :, : lens[b] + 2 * self.ctx])[0].t() for b in range(B)])
        skips = residual_stack(self.plan(), self.maps(n_of), x0.contiguous(), cu.contiguous(), [blk.plain() for blk in self.conv_layers])
        l1, l3 = self.last_conv_layers[1], self.last_conv_layers[3]
        y = F.linear(torch.relu(skips * math.sqrt(1.0 / self.config["layers"])), l1.folded()[:, :, 0], l1.bias)
        y = F.linear(torch.relu(y), l3.folded()[:, :, 0], l3.bias)[:, 0]
        if lens is None:
            return y.reshape(B, 1, T)
        rows, off = [], 0
        for n in n_of:
            rows.append(F.pad(y[off : off + n], (0, T - n)))
            off += n
        return torch.stack(rows).unsqueeze(1)

    def _forward_hip(self, z, c, lens, B, T):
        plan = self.plan()
        check_ends(self.scales, self.ctx)
        if lens is None:
            maps = self.maps([T] * B)
            zp, cp = z.reshape(B * T), c.transpose(1, 2).reshape(-1, c.shape[1])
        else:
            lens = [int(n) for n in lens]
            if len(lens) != B or min(lens) < 1 or max(lens) * self.hop > T:
                raise ValueError("fcl-taco2_amd: PWG generator: lens %r (frames) do not fit %d samples at hop %d" % (lens, T, self.hop))
            maps = self.maps([n * self.hop for n in lens])
            zr, cr = maps.rows(T, self.ctx)
            zp, cp = z.reshape(B * T)[zr], c.transpose(1, 2).reshape(-1, c.shape[1])[cr]
        up, l1, l3 = self.upsample_net.upsample.up_layers, self.last_conv_layers[1], self.last_conv_layers[3]
        cu, x0 = input_end(plan, maps, zp, cp, self.upsample_net.conv_in.folded(), [up[2 * i + 1].folded() for i in range(len(self.scales))],
                           self.first_conv.folded(), self.first_conv.bias)
        skips = residual_stack(plan, maps, x0, cu, [blk.plain() for blk in self.conv_layers])
        y = output_end(plan, maps, skips, l1.folded(), l1.bias, l3.folded(), l3.bias)
        if lens is None:
            return y.reshape(B, 1, T)
        return torch.zeros(B * T, device=y.device, dtype=y.dtype).index_copy(0, zr, y).reshape(B, 1, T)
