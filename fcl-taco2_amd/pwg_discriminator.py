"""The Parallel WaveGAN discriminator on the HIP path, with its backward pass (the pwd_* kernels of csrc/pwg_disc.hip).

A stack of `layers` Conv1d on the waveform: layer 0 is 1 -> C with dilation 1, layers 1 .. layers - 2 are C -> C with dilation i (or dilation_factor ** i),
each followed by LeakyReLU, and the last layer is C -> 1 with dilation 1 and no activation; padding (k - 1) / 2 * d keeps the length.  The published
architecture (Yamamoto et al. 2020); parity with the parallel_wavegan package's checkpoints is by parameter names and layout, not pinned against its code.

    disc = ParallelWaveGANDiscriminator().to("cuda:0")
    p = disc(wave)                       # [B, T], [B, 1, T] -> [B, 1, T] scores; packed 1-D with lens= -> packed 1-D scores
    generator_adversarial_loss(disc(fake)).backward()

The contract is stated in include/fcl_hip.h "Parallel WaveGAN discriminator" and restated in float64 numpy in tests/pwgd_ref.py.  Activations are float32,
channel-last [samples, C], the batch packed with the utterances back to back; only the post-activations are kept for the backward pass.  One arithmetic
mode (exact fp32).  No CPU fallback."""
import ctypes as C

import torch

from . import _lib, ops
from .pwg_common import MAX_SAMPLES, Maps, _Conv, _Module  # noqa: F401 (Maps: the packed batch's seg_lo / seg_hi, used through this module too)

KERNEL_SIZES = (3, 5)


def check_configuration(in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1, nonlinear_activation="LeakyReLU",
                        negative_slope=0.2, bias=True, use_weight_norm=True):
    """-> [(cin, cout, dilation)] per layer; anything the kernels do not cover is refused by the argument's name"""
    bad = lambda name, got, want: ValueError("fcl-taco2_amd: PWG discriminator: %s=%r is not supported on the HIP path (%s)" % (name, got, want))
    if in_channels != 1:
        raise bad("in_channels", in_channels, "1")
    if out_channels != 1:
        raise bad("out_channels", out_channels, "1")
    if kernel_size not in KERNEL_SIZES:
        raise bad("kernel_size", kernel_size, "3 or 5")
    if not (isinstance(layers, int) and 3 <= layers <= 16):
        raise bad("layers", layers, "3 to 16")
    if not (isinstance(conv_channels, int) and 16 <= conv_channels <= 128 and conv_channels % 16 == 0):
        raise bad("conv_channels", conv_channels, "a multiple of 16 from 16 to 128")
    if not (isinstance(dilation_factor, int) and dilation_factor >= 1):
        raise bad("dilation_factor", dilation_factor, "an integer >= 1")
    if nonlinear_activation != "LeakyReLU":
        raise bad("nonlinear_activation", nonlinear_activation, "LeakyReLU")
    if not 0.0 <= float(negative_slope) < 1.0:
        raise bad("negative_slope", negative_slope, "0 <= negative_slope < 1")
    if bias not in (True, False):
        raise bad("bias", bias, "True or False")
    if use_weight_norm not in (True, False):
        raise bad("use_weight_norm", use_weight_norm, "True or False")
    geo = []
    for i in range(layers - 1):
        d = 1 if i == 0 else (i if dilation_factor == 1 else dilation_factor ** i)
        if d > MAX_SAMPLES:
            raise bad("dilation_factor", dilation_factor, "dilation_factor ** (layers - 2) below 2^31")
        geo.append((1 if i == 0 else conv_channels, conv_channels, d))
    geo.append((conv_channels, 1, 1))
    return geo


class DiscriminatorPlan(object):
    """Per-layer geometry (cin, cout, dilation) and the sizes of what a pass needs for n samples"""

    def __init__(self, device="cuda:0", **config):
        self.geometry = check_configuration(**config)
        cfg = dict(kernel_size=3, layers=10, conv_channels=64, dilation_factor=1, negative_slope=0.2, bias=True)
        cfg.update({k: v for k, v in config.items() if k in cfg})
        self.kernel_size, self.layers, self.channels = cfg["kernel_size"], cfg["layers"], cfg["conv_channels"]
        self.slope, self.bias = float(cfg["negative_slope"]), bool(cfg["bias"])
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: DiscriminatorPlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)
        self.receptive_field = 1 + (self.kernel_size - 1) * sum(d for _, _, d in self.geometry)

    def act_shapes(self, n):
        """the activations of a pass over n samples: h_0 .. h_{layers - 2} [n, C] and the scores [n]"""
        return [(n, self.channels)] * (self.layers - 1) + [(n,)]

    def grad_floats(self, n):
        """each of the two alternating gradient buffers of the backward pass"""
        return n * self.channels

    def workspace_floats(self, n):
        """the partials of the largest layer's weight gradient"""
        lib = _lib.load()
        return max(lib.fcl_pwd_dw_workspace_bytes(n, ci, co, self.kernel_size) for ci, co, _ in self.geometry) // 4

    def dweight_shapes(self):
        """per layer (dw [k, cin, cout], db [cout]) in the kernels' tap-major layout"""
        return [((self.kernel_size, ci, co), (co,)) for ci, co, _ in self.geometry]


def pack_weights(weights, biases):
    """torch Conv1d weights [cout, cin, k] -> per layer (wf [k, cin, cout], wb [k, cout, cin] with the taps reversed, bias or None), contiguous"""
    out = []
    for w, b in zip(weights, biases):
        w = w.detach().to(torch.float32)
        out.append((w.permute(2, 1, 0).contiguous(), w.flip(2).permute(2, 0, 1).contiguous(), None if b is None else b.detach().to(torch.float32).contiguous()))
    return out


def unpack_dweight(dw):
    """the kernels' [k, cin, cout] -> torch's [cout, cin, k]"""
    return dw.permute(2, 1, 0).contiguous()


def _args(plan, maps, layer, **ptr):
    ci, co, d = plan.geometry[layer]
    a = _lib.PwdLayer()
    a.samples, a.cin, a.cout, a.ksize, a.dilation, a.slope = maps.samples, ci, co, plan.kernel_size, d, plan.slope
    a.seg_lo, a.seg_hi = maps.seg_lo.data_ptr(), maps.seg_hi.data_ptr()
    for k, v in ptr.items():
        if v is not None:
            setattr(a, k, v.data_ptr())
    return a


# on caller-owned buffers (the tests surround them with guard zones)
def launch_forward(plan, maps, x, weights, acts):
    """x [samples] float32, weights from pack_weights -> acts: h_0 .. h_{layers - 2} [samples, C] and the scores [samples] (plan.act_shapes)"""
    lib, st = _lib.load(), ops._stream()
    src = x
    for l, (wf, _, b) in enumerate(weights):
        _lib.check(lib.fcl_pwd_layer_fwd(C.byref(_args(plan, maps, l, x=src, w=wf, bias=b, y=acts[l])), st))
        src = acts[l]


def launch_backward(plan, maps, dscore, weights, acts, gx, dweights, x=None, grads=None, workspace=None):
    """dscore [samples] -> gx [samples] (None: the waveform gradient is not computed) and dweights = [(dw [k, cin, cout], db [cout] or None)] per layer
    (None: no weight gradient is computed).  x: the waveform (needed with dweights); grads: two buffers of plan.grad_floats(samples) floats; workspace:
    plan.workspace_floats(samples) floats (needed with dweights)."""
    lib, st = _lib.load(), ops._stream()
    g = dscore
    for l in range(plan.layers - 1, -1, -1):
        wf, wb, _ = weights[l]
        below = x if l == 0 else acts[l - 1]
        if dweights is not None:
            dw, db = dweights[l]
            a = _args(plan, maps, l, x=below, g=g, dw=dw, db=db, workspace=workspace)
            a.workspace_bytes = workspace.numel() * 4
            _lib.check(lib.fcl_pwd_layer_dw(C.byref(a), st))
        if l > 0:
            out = grads[l & 1][: maps.samples * plan.channels]
            _lib.check(lib.fcl_pwd_layer_dx(C.byref(_args(plan, maps, l, g=g, w=wb, h=below, y=out)), st))
            g = out
        elif gx is not None:
            _lib.check(lib.fcl_pwd_layer_dx(C.byref(_args(plan, maps, l, g=g, w=wb, y=gx)), st))


class _Function(torch.autograd.Function):
    """scores of the packed waveform under plain weights and biases; backward gives the gradients of all of them that are asked for"""

    @staticmethod
    def forward(ctx, plan, maps, x, *params):
        L, dev, n = plan.layers, plan.device, maps.samples
        ws, bs = params[:L], params[L:] if plan.bias else [None] * L
        with torch.cuda.device(dev):
            x = x.detach().contiguous()
            packed = pack_weights(ws, bs)
            acts = [torch.empty(s, device=dev, dtype=torch.float32) for s in plan.act_shapes(n)]
            launch_forward(plan, maps, x, packed, acts)
        ctx.plan, ctx.maps, ctx.packed, ctx.acts, ctx.x = plan, maps, packed, acts[:-1], x
        return acts[-1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dscore):
        plan, maps, dev, n = ctx.plan, ctx.maps, ctx.plan.device, ctx.maps.samples
        need_x, need_w = ctx.needs_input_grad[2], any(ctx.needs_input_grad[3:])
        with torch.cuda.device(dev):
            new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
            gx = new(n) if need_x else None
            dweights = [(new(sw), new(sb) if plan.bias else None) for sw, sb in plan.dweight_shapes()] if need_w else None
            launch_backward(plan, maps, dscore.detach().to(torch.float32).contiguous(), ctx.packed, ctx.acts + [None], gx, dweights, x=ctx.x,
                            grads=[new(plan.grad_floats(n)), new(plan.grad_floats(n))], workspace=new(plan.workspace_floats(n)) if need_w else None)
        out = [None, None, gx]
        if need_w:
            out += [unpack_dweight(dw) for dw, _ in dweights] + ([db for _, db in dweights] if plan.bias else [])
        else:
            out += [None] * (len(ctx.needs_input_grad) - 3)
        return tuple(out)


class _Activation(torch.nn.Module):  # holds the odd indices of conv_layers, as the reference's Sequential of conv, activation, conv, ...
    pass


class ParallelWaveGANDiscriminator(_Module):
    """forward(x, lens=None) -> scores.  Parameters: conv_layers.{2 i}.weight / .bias (weight_g / weight_v under use_weight_norm), the last convolution at
    index 2 (layers - 1); Kaiming-normal weights, zero biases."""

    CHECKPOINT_KEY, PLAN = "discriminator", DiscriminatorPlan

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params=None, bias=True, use_weight_norm=True, negative_slope=None):
        super().__init__()
        params = dict(nonlinear_activation_params or {"negative_slope": 0.2})
        if negative_slope is not None:
            params["negative_slope"] = negative_slope
        extra = sorted(set(params) - {"negative_slope", "inplace"})
        if extra:
            raise ValueError("fcl-taco2_amd: PWG discriminator: nonlinear_activation_params=%r is not supported on the HIP path (negative_slope only)" % (extra,))
        self.config = dict(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, layers=layers, conv_channels=conv_channels,
                           dilation_factor=dilation_factor, nonlinear_activation=nonlinear_activation, negative_slope=params.get("negative_slope", 0.01),
                           bias=bias, use_weight_norm=use_weight_norm)
        geo = check_configuration(**self.config)
        mods = []
        for i, (ci, co, _) in enumerate(geo):
            mods.append(_Conv((co, ci, kernel_size), bias, use_weight_norm))
            if i < layers - 1:
                mods.append(_Activation())
        self.conv_layers = torch.nn.ModuleList(mods)
        self.use_weight_norm = bool(use_weight_norm)
        self._reset_cache()

    def convs(self):
        return [m for m in self.conv_layers if isinstance(m, _Conv)]

    def pack(self, x, lens=None):
        """-> (packed x, lens, the shape to give back); torch operations, so the padding of a [B, T] input with lens gets zero gradient"""
        dev = self.plan().device
        x = torch.as_tensor(x)
        if x.dim() == 3:
            if x.shape[1] != 1:
                raise ValueError("fcl-taco2_amd: PWG discriminator: a 3-D input must be [B, 1, T], got %r" % (tuple(x.shape),))
            x = x[:, 0]
        x = x.to(device=dev, dtype=torch.float32)
        if x.dim() == 1:
            lens = [int(x.numel())] if lens is None else [int(n) for n in lens]
            if sum(lens) != x.numel():
                raise ValueError("fcl-taco2_amd: PWG discriminator: the packed waveform has %d samples, lens sum to %d" % (x.numel(), sum(lens)))
            return x.contiguous(), lens, None
        if x.dim() != 2:
            raise ValueError("fcl-taco2_amd: PWG discriminator: [B, T], [B, 1, T] or packed 1-D input expected, got %r" % (tuple(x.shape),))
        B, T = x.shape
        if lens is None:
            return x.reshape(-1).contiguous(), [int(T)] * int(B), (int(B), 1, int(T))
        lens = [int(n) for n in lens]
        if len(lens) != B or max(lens) > T or min(lens) < 1:
            raise ValueError("fcl-taco2_amd: PWG discriminator: lens %r do not fit an input of %r" % (lens, tuple(x.shape)))
        return torch.cat([x[b, :n] for b, n in enumerate(lens)]).contiguous(), lens, None

    def forward(self, x, lens=None):
        x, lens, shape = self.pack(x, lens)
        convs = self.convs()
        params = [m.folded() for m in convs] + ([m.bias for m in convs] if self.config["bias"] else [])
        p = _Function.apply(self.plan(), self.maps(lens), x, *params)
        return p if shape is None else p.reshape(shape)


def generator_adversarial_loss(p_fake):
    """parallel_wavegan's MSE form: mean (p - 1)^2"""
    return torch.mean((p_fake - 1.0) ** 2)


def discriminator_adversarial_loss(p_real, p_fake):
    """-> (real loss, fake loss) = (mean (p_real - 1)^2, mean p_fake^2)"""
    return torch.mean((p_real - 1.0) ** 2), torch.mean(p_fake ** 2)
