"""The rest of the names `lic360_operator/__init__.py:1-29` exports, so that `test/lic360_demo.py:3-4` and
`test/model_zoo.py:3` import unchanged.  They sit OUTSIDE the accelerated path (pure-torch activation /
metric / bookkeeping utilities, and two wrappers of out-of-scope native ops) and are plain PyTorch-ROCm here:

  GDN            generalized divisive normalisation, y = x / sqrt(beta + sum_j gamma_ij x_j^2) (lic360_operator/GDN.py:26-100):
                 same constructor, parameter names (`beta`, `gamma`) and reparametrisation, so checkpoints load.
  DropGrad       identity with a gradient gate (lic360_operator/DropGrad.py:4-24)
  SSIM           11x11 Gaussian-window SSIM (lic360_operator/pytorch_ssim.py:16-63)
  ModuleSaver    best / latest checkpoint writer (lic360_operator/ModuleSaver.py:4-35)
  Logger         screen + file log (lic360_operator/Logger.py:3-23)
  MultiProject   the 14 viewports of lic360.ProjectsOp (viewport metrics)
  ViewportQuality  viewport MSE / SSIM per image and viewport: one fused native pass (lic360.viewport_quality), MultiProject + SSIM elsewhere;
                 not a name of the reference
  GmmRateLoss    the rate term of the training loss from the three entropy nets' raw outputs: one fused native pass each way (lic360.gmm_rate,
                 autograd.GmmRateFn), or ContextReshape + softmax + ReLU + EntropyGmm + mask + sum; not a name of the reference
  CeRateLoss     the rate term of the importance map's entropy model from its net's raw output: one fused native pass each way (lic360.ce_rate,
                 autograd.CeRateFn), or ContextReshape + cross_entropy + sum; not a name of the reference
  MaskConv2      torch conv2d over a weight masked by lic360.MaskConstrainOp (the training-time form of the context conv)
"""
import math
import os

import torch
from torch import nn
import torch.nn.functional as F


class _FloorSTE(torch.autograd.Function):
    """max(x, bound) whose gradient also passes where it would move x back above the bound."""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x)
        ctx.bound = float(bound)
        return x.clamp_min(ctx.bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        keep = (x >= ctx.bound) | (g < 0)
        return g * keep.to(g.dtype), None


class GDN(nn.Module):
    """grad: where a pass that records gradients goes.  "library" (the default): the reference's composition -- x * x, a 1x1 conv2d, sqrt and a
    division or product -- and autograd's chain through it, which keeps x^2 and the norm for the backward.  "fused" (opt-in): an fp32 CUDA tensor of
    a channel count the one-pass kernel takes goes through autograd.GdnFn -- lic360.gdn_forward, then lic360.gdn_backward, which recomputes the
    norm and keeps nothing but x; CPU tensors, other dtypes and other channel counts still take the composition.  Under "fused" the recording
    forward is the fp32 kernel whatever `_gdn_precision` says (the backward's recomputed sum is then the forward's, bit for bit), and it returns
    the bits the fp32 inference forward returns.  The reparametrisation of beta and gamma is torch work on both routes; state dict, parameter names
    and shapes do not depend on the route.  The attribute can be switched between calls (lic360_models.set_gdn_grad does it for a whole model).
    Measured (tools/gdn_grad_probe.py, DESIGN.md "Native backward of the one-pass GDN"): the table there says what the fused route buys and why
    "library" stays the default."""
    GRADS = ("library", "fused")

    def __init__(self, ch, device=0, inverse=False, beta_min=1e-6, gamma_init=.1, reparam_offset=2 ** -18, grad="library"):
        super().__init__()
        self.grad = self._grad(grad)
        self.inverse = bool(inverse)
        dev = torch.device("cuda:%d" % (device if isinstance(device, int) else device[0])) if torch.cuda.is_available() else torch.device("cpu")
        ped = float(reparam_offset) ** 2
        self.pedestal = ped
        self.beta_bound = math.sqrt(float(beta_min) + ped)
        self.gamma_bound = float(reparam_offset)
        self.beta = nn.Parameter(torch.sqrt(torch.ones(ch) + ped).to(dev))
        self.gamma = nn.Parameter(torch.sqrt(float(gamma_init) * torch.eye(ch) + ped).to(dev))

    @classmethod
    def _grad(cls, grad):
        if grad not in cls.GRADS:
            raise ValueError("GDN: grad must be one of %s, got %r" % (", ".join(repr(g) for g in cls.GRADS), grad))
        return grad

    def _fused_backward(self, x):
        """does this call record gradients on a tensor the native forward and backward take?"""
        if not (torch.is_grad_enabled() and (x.requires_grad or self.beta.requires_grad or self.gamma.requires_grad)):
            return False
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3 and x.numel() > 0):
            return False
        import lic360
        return lic360.gdn_supported(x.shape[1])

    def forward(self, x):
        if getattr(self, "grad", "library") == "fused" and self._fused_backward(x):
            from .autograd import GdnFn
            beta = _FloorSTE.apply(self.beta.to(x.device), self.beta_bound) ** 2 - self.pedestal
            gamma = _FloorSTE.apply(self.gamma.to(x.device), self.gamma_bound) ** 2 - self.pedestal
            return GdnFn.apply(x.contiguous(), gamma, beta, self.inverse)
        shape = x.shape
        if x.dim() == 5:
            x = x.reshape(shape[0], shape[1], shape[2] * shape[3], shape[4])
        ch = x.shape[1]
        beta = _FloorSTE.apply(self.beta.to(x.device), self.beta_bound) ** 2 - self.pedestal
        gamma = _FloorSTE.apply(self.gamma.to(x.device), self.gamma_bound) ** 2 - self.pedestal
        if not (torch.is_grad_enabled() and (x.requires_grad or self.beta.requires_grad)) and x.is_cuda and x.dtype == torch.float32:
            import lic360
            if getattr(self, "_gdn_precision", "fp32") == "bf16x3" and lic360.gdn_bf16x3_supported(ch):
                return lic360.gdn_bf16x3_forward(x.contiguous(), self._gdn_b3_pack(lic360, gamma.detach()), beta.detach(), self.inverse).reshape(shape)
            if lic360.gdn_supported(ch):                                    # one fused pass instead of four torch kernels
                return lic360.gdn_forward(x.contiguous(), gamma.detach(), beta.detach(), self.inverse).reshape(shape)
        norm = torch.sqrt(F.conv2d(x * x, gamma.view(ch, ch, 1, 1), beta))
        y = x * norm if self.inverse else x / norm
        return y.reshape(shape)

    def _gdn_b3_pack(self, lic360, gamma):
        """the effective gamma in the split-bf16 kernel's operand order, repacked when the parameter was written (its version counter) or moved"""
        key = (self.gamma.data_ptr(), self.gamma._version, gamma.device)
        if getattr(self, "_gdn_b3_packed", (None, None))[0] != key:
            self._gdn_b3_packed = (key, lic360.gdn_bf16x3_pack(gamma))
        return self._gdn_b3_packed[1]


class _GradGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep):
        ctx.keep = keep
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.keep, None


class DropGrad(nn.Module):
    def __init__(self, drop=True):
        super().__init__()
        self.drop = 0 if drop else 1            # multiplier of the incoming gradient

    def forward(self, x):
        return _GradGate.apply(x, self.drop)


def _gauss_taps(size, sigma=1.5):
    k = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-k * k / (2.0 * sigma * sigma))
    return g / g.sum()


def _gauss_window(size, channel, sigma=1.5):
    g = _gauss_taps(size, sigma)
    return (g[:, None] * g[None, :]).expand(channel, 1, size, size).contiguous()


class SSIM(nn.Module):
    def __init__(self, window_size=11, channel=1, size_average=True):
        super().__init__()
        self.window_size, self.channel, self.size_average = int(window_size), int(channel), bool(size_average)
        self.window = _gauss_window(self.window_size, self.channel)

    def map(self, a, b):
        """the per-cell SSIM, before any mean"""
        ch = a.shape[1]
        if ch != self.channel or self.window.device != a.device or self.window.dtype != a.dtype:
            self.window, self.channel = _gauss_window(self.window_size, ch).to(device=a.device, dtype=a.dtype), ch
        w, p = self.window, self.window_size // 2
        blur = lambda t: F.conv2d(t, w, padding=p, groups=ch)
        mu_a, mu_b = blur(a), blur(b)
        var_a, var_b, cov = blur(a * a) - mu_a * mu_a, blur(b * b) - mu_b * mu_b, blur(a * b) - mu_a * mu_b
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        return ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))

    def forward(self, a, b):
        m = self.map(a, b)
        return m.mean() if self.size_average else m.mean(dim=(1, 2, 3))


class ModuleSaver(object):
    """save(model, loss) keeps `<prex>_best_<i>.pt` per tracked loss and `<prex>_latest.pt` otherwise."""

    def __init__(self, path="./saved_models/", prex="default"):
        self.path, self.prex = path, prex
        os.makedirs(path, exist_ok=True)
        self.current_best_loss, self.init = None, False

    def init_loss(self, loss):
        self.current_best_loss = list(loss) if isinstance(loss, list) else [loss]
        self.init = True

    def save(self, model, loss):
        wrapped = isinstance(model, (nn.DataParallel, nn.parallel.DistributedDataParallel))
        state = (model.module if wrapped else model).state_dict()
        loss = loss if isinstance(loss, list) else [loss]
        if not self.init:
            self.init_loss([10e9] * len(loss))
        msg = ""
        for i, v in enumerate(loss):
            if v < self.current_best_loss[i]:
                self.current_best_loss[i] = v
                torch.save(state, os.path.join(self.path, "%s_best_%d.pt" % (self.prex, i)))
                msg += "save %s_best_%d.pt\t" % (self.prex, i)
        if not msg:
            torch.save(state, os.path.join(self.path, "%s_latest.pt" % self.prex))
            msg = "update %s_latest.pt" % self.prex
        return msg


class Logger(object):
    def __init__(self, fname, screen=True, file=True):
        self.screen_out, self.file = screen, file
        self.fout = open(fname, "w") if file else None

    def log(self, *args):
        if self.screen_out:
            print(*args)
        if self.fout:
            self.fout.write(" ".join(str(a) for a in args) + "\n")
            self.fout.flush()

    def close(self):
        if self.fout:
            self.fout.close()
            self.fout = None

    def __del__(self):
        self.close()


class MultiProject(nn.Module):
    """14 viewports of every ERP image of a batch -- four around the equator, four each at +-45 degrees, the two poles -- for the
    viewport metrics (reference lic360_operator/MultiProject.py:24-35; used as `MultiProject(171, 256, 0.5, False, gpu)` by
    test/lic360_demo.py:424-425).  Output [n*14, c, h, w], viewport-major."""
    THETAS = (-0.5, 0, 0.5, 1, -0.5, 0, 0.5, 1, -0.5, 0, 0.5, 1, 0, 0)
    PHIS = (0, 0, 0, 0, 0.25, 0.25, 0.25, 0.25, -0.25, -0.25, -0.25, -0.25, 0.5, -0.5)

    def __init__(self, h, w, fov=0.6, near=False, device_id=0, time_flag=False):
        super().__init__()
        import lic360
        from .autograd import UnaryFn, recording
        self._fn, self._recording = UnaryFn, recording
        self.thetas, self.phis = list(self.THETAS), list(self.PHIS)
        devs = [device_id] if isinstance(device_id, int) else list(device_id)
        self.op = {gid: lic360.ProjectsOp(int(h), int(w), self.thetas, self.phis, fov, near, gid, time_flag) for gid in devs}

    def forward(self, x):
        x = x if x.is_contiguous() else x.contiguous()
        op = self.op[x.device.index]
        if self._recording(x):
            return self._fn.apply(x, op, False)
        with torch.no_grad():
            return op.forward(x)[0]


class ViewportQuality(nn.Module):
    """The viewport metrics of the evaluation mode (test/lic360_demo.py:406-449: `MultiProject(171, 256, 0.5, False, gpu)`, `SSIM(11, 3)` and
    an MSE on the views) per image and viewport: forward(a, b) -> (mse, ssim), each [n, 14] fp32; `mse.mean()` and `ssim.mean()` are the
    reference's two scalars (every viewport has the same number of cells).  fp32 contiguous tensors on the device, outside a recording
    pass, take one fused native pass (lic360.viewport_quality) that writes no projected view; with return_map=True it also returns the
    per-cell SSIM [14*n, c, h, w], viewport-major.  Anything else -- CPU tensors, other dtypes, strided tensors, a pass that records
    gradients -- goes through MultiProject + SSIM + torch.mean and is reduced per (image, viewport) there: the module takes tensors of any
    placement and dtype, but the projection is native in both paths, so a HIP device is needed either way (CPU tensors are projected on
    `device_id` and the results come back to the CPU).
    grad: where a pass that records gradients goes.  "library" (the default): the library path above, as before.  "fused" (opt-in): fp32
    contiguous device tensors without return_map take autograd.ViewportQualityFn -- the fused forward that also keeps four coefficient maps, and
    one fused backward kernel (lic360.viewport_quality_coef / viewport_quality_backward); everything else still takes the library path.  The
    attribute can be switched between calls."""
    GRAD_MODES = ("library", "fused")

    def __init__(self, h, w, fov=0.5, near=False, device_id=0, window_size=11, grad="library"):
        super().__init__()
        self.grad = self._grad_mode(grad)
        self.project = MultiProject(h, w, fov, near, device_id)
        self.window_size = int(window_size)
        self.ssim = SSIM(self.window_size, 3)
        self.taps = _gauss_taps(self.window_size).tolist()
        self.device_id = device_id if isinstance(device_id, int) else list(device_id)[0]

    @classmethod
    def _grad_mode(cls, mode):
        if mode not in cls.GRAD_MODES:
            raise ValueError("ViewportQuality: grad must be one of %s, got %r" % (", ".join(repr(m) for m in cls.GRAD_MODES), mode))
        return mode

    def _views(self, t, dev):
        """the op owns its output -- the next call rewrites it (the caller clones) -- and a recorded pass leaves its graph node on that tensor"""
        v = self.project(t.to(device=dev, dtype=torch.float32))
        return v if self.project._recording(t) else v.detach()

    def forward(self, a, b, return_map=False):
        if a.shape != b.shape or a.dim() != 4:
            raise ValueError("ViewportQuality takes two [n, c, h, w] tensors of one shape")
        import lic360
        native = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (a, b)) and a.device == b.device and a.device.index in self.project.op
        recording = self.project._recording(a, b)
        if native and not recording:
            return lic360.viewport_quality(self.project.op[a.device.index], a, b, self.taps, return_map=return_map)
        if native and not return_map and self._grad_mode(getattr(self, "grad", "library")) == "fused":
            from .autograd import ViewportQualityFn
            return ViewportQualityFn.apply(a, b, self.project.op[a.device.index], self.taps)
        dev = a.device if a.is_cuda and a.device.index in self.project.op else torch.device("cuda:%d" % self.device_id)
        n = a.shape[0]
        va, vb = self._views(a, dev).clone(), self._views(b, dev)                               # [14 n, c, h, w], viewport-major
        m = self.ssim.map(va, vb)
        per_view = lambda t: t.mean(dim=(1, 2, 3)).view(14, n).t().contiguous().to(a.device)
        mse, ssim = per_view((va - vb) ** 2), per_view(m)
        return (mse, ssim, m.to(a.device)) if return_map else (mse, ssim)


class GmmRateLoss(nn.Module):
    """The rate term of the training objective from the raw outputs of the three entropy nets (reference train/EntropyNet2.py:67-74 and
    train/model_zoo.py:295-296): forward(logit, sigma, mean, label, mask=None, return_map=False) -> (nats [n] float64, symbols [n] int64), plus
    the per-symbol loss [n, g, h, w] (0 where uncoded) with return_map.  logit, sigma, mean [n, ngroup * num_gaussian, h, w]; label, mask
    [n, ngroup, h, w]; symbol (n, g, y, x) reads channel g * num_gaussian + i of each net.
    route "library": the composition the reference trains with on this package's modules -- ContextReshape x 3, torch.softmax, relu, + 1e-5,
    EntropyGmm, the product with the mask, a per-image sum in float64; symbols counts mask >= 0.5.  It takes tensors of any placement and
    dtype (they are computed in fp32 on `device_id`, the results come back to the inputs' device).
    route "fused": fp32 contiguous device tensors take one native pass -- lic360.gmm_rate without a recording pass, autograd.GmmRateFn (which
    saves the inputs only and runs lic360.gmm_rate_backward) with one; a symbol is coded iff mask >= 0.5, the coder's rule, which is the
    product for 0 / 1 masks.  CPU tensors, other dtypes, strided tensors and a recording call with return_map=True take the library route.
    The attribute can be switched between calls."""
    ROUTES = ("library", "fused")

    def __init__(self, ngroup, num_gaussian=3, route="fused", device_id=0):
        super().__init__()
        from .quantize import ContextReshape
        from .tables import EntropyGmm
        from .autograd import recording
        self.ngroup, self.num_gaussian, self.route = int(ngroup), int(num_gaussian), self._route(route)
        self.device_id = device_id if isinstance(device_id, int) else list(device_id)[0]
        self._recording = recording
        # one reshape op per net: an op owns its output, the next call of the same op rewrites it
        self.reshape = nn.ModuleList([ContextReshape(self.ngroup, device_id) for _ in range(3)])
        self.ent_loss = EntropyGmm(self.num_gaussian, device=device_id)

    @classmethod
    def _route(cls, route):
        if route not in cls.ROUTES:
            raise ValueError("GmmRateLoss: route must be one of %s, got %r" % (", ".join(repr(r) for r in cls.ROUTES), route))
        return route

    def loss_vec(self, logit, sigma, mean, label):
        """the reference's per-symbol loss_vec [n * ngroup * h * w] of fp32 device tensors, before any mask (the library composition)"""
        weight = torch.softmax(self.reshape[0](logit), dim=1)
        delta = torch.relu(self.reshape[1](sigma)) + 0.00001
        return self.ent_loss(weight, delta, self.reshape[2](mean), label.reshape(-1, 1))

    def _library(self, logit, sigma, mean, label, mask, return_map):
        dev = logit.device if logit.is_cuda else torch.device("cuda:%d" % self.device_id)
        f = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32)
        vec = self.loss_vec(f(logit), f(sigma), f(mean), f(label))
        n = label.shape[0]
        if mask is None:
            symbols = torch.full((n,), label[0].numel() if n else 0, dtype=torch.int64, device=logit.device)
        else:
            vec = vec * f(mask).reshape(-1)
            symbols = (mask.reshape(n, -1) >= 0.5).sum(1).to(logit.device)
        nats = vec.view(n, -1).double().sum(1).to(logit.device)
        return (nats, symbols, vec.view(label.shape).to(logit.device)) if return_map else (nats, symbols)

    def forward(self, logit, sigma, mean, label, mask=None, return_map=False):
        if label.dim() != 4 or label.shape[1] != self.ngroup or logit.dim() != 4 or logit.shape[1] != self.ngroup * self.num_gaussian or \
                logit.shape != sigma.shape or logit.shape != mean.shape or (mask is not None and mask.shape != label.shape) or \
                (logit.shape[0],) + tuple(logit.shape[2:]) != (label.shape[0],) + tuple(label.shape[2:]):
            raise ValueError("GmmRateLoss takes logit, sigma, mean [n, %d, h, w] and label, mask [n, %d, h, w]" % (self.ngroup * self.num_gaussian, self.ngroup))
        ts = [t for t in (logit, sigma, mean, label, mask) if t is not None]
        native = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == logit.device for t in ts) and label.numel() > 0
        recording = self._recording(logit, sigma, mean, label)
        if self._route(getattr(self, "route", "library")) == "fused" and native and not (recording and return_map):
            import lic360
            if not recording:
                return lic360.gmm_rate(logit, sigma, mean, label, mask, return_map=return_map, ngroup=self.ngroup)
            from .autograd import GmmRateFn
            return GmmRateFn.apply(logit, sigma, mean, label, mask)
        return self._library(logit, sigma, mean, label, mask, return_map)


class CeRateLoss(nn.Module):
    """The rate term of the importance map's entropy model from the raw output of its net (reference test/model_zoo.py:275-300: ContextReshape,
    then CrossEntropyLoss over nclass classes): forward(logit, label, return_map=False) -> (nats [n] float64, symbols [n] int64), plus the
    per-symbol loss [n, g, h, w] with return_map.  logit [n, ngroup * nclass, h, w]; label [n, ngroup, h, w] holding class indices; symbol
    (n, g, y, x) reads channel g * nclass + i; its class is the label truncated, as the reference's `.type(torch.LongTensor)` does.
    route "library": the composition the reference trains with on this package's modules -- ContextReshape,
    torch.nn.functional.cross_entropy(..., reduction="none") (`loss_vec`), a per-image sum in float64; symbols counts every symbol.  It takes
    tensors of any placement and dtype (they are computed in fp32 on `device_id`, the results come back to the inputs' device); a label outside
    0 .. nclass - 1 raises through torch.
    route "fused": fp32 contiguous device tensors take one native pass -- lic360.ce_rate without a recording pass, autograd.CeRateFn (which saves
    the inputs only and runs lic360.ce_rate_backward) with one.  A label outside (-1, nclass), NaN included, costs nothing, gets a zero gradient
    and is counted out of symbols; with check_labels (the default) the call then raises IndexError, which costs one synchronisation;
    check_labels=False skips the check.  CPU tensors, other dtypes, strided tensors and a recording call with return_map=True take the library
    route.  The attribute can be switched between calls.
    The default is "library": measured at 1 x 64 x 128, 49 classes (tools/ce_rate_probe.py), the fused route's medians are 1.1 - 1.2 x lower at batch 8
    and batch 1, forward and forward + backward, but only two of the four differences exceed the two min - max spreads added -- both routes are bound
    by the host at 0.05 - 0.25 ms per call, the fused entries alone take at most 0.016 + 0.017 ms of it -- so the rule that made "fused" GmmRateLoss's
    default does not."""
    ROUTES = ("library", "fused")

    def __init__(self, ngroup, nclass, route="library", device_id=0, check_labels=True):
        super().__init__()
        from .quantize import ContextReshape
        from .autograd import recording
        self.ngroup, self.nclass, self.route, self.check_labels = int(ngroup), int(nclass), self._route(route), bool(check_labels)
        self.device_id = device_id if isinstance(device_id, int) else list(device_id)[0]
        self._recording = recording
        self.reshape = ContextReshape(self.ngroup, device_id)

    @classmethod
    def _route(cls, route):
        if route not in cls.ROUTES:
            raise ValueError("CeRateLoss: route must be one of %s, got %r" % (", ".join(repr(r) for r in cls.ROUTES), route))
        return route

    def loss_vec(self, logit, label):
        """the reference's per-symbol loss_vec [n * ngroup * h * w] of fp32 device tensors (the library composition)"""
        return F.cross_entropy(self.reshape(logit), label.reshape(-1).to(torch.int64), reduction="none")

    def _library(self, logit, label, return_map):
        dev = logit.device if logit.is_cuda else torch.device("cuda:%d" % self.device_id)
        f = lambda t: t.to(device=dev, dtype=torch.float32)
        vec = self.loss_vec(f(logit), f(label))
        n = label.shape[0]
        symbols = torch.full((n,), label[0].numel() if n else 0, dtype=torch.int64, device=logit.device)
        nats = vec.view(n, -1).double().sum(1).to(logit.device)
        return (nats, symbols, vec.view(label.shape).to(logit.device)) if return_map else (nats, symbols)

    def forward(self, logit, label, return_map=False):
        if label.dim() != 4 or label.shape[1] != self.ngroup or logit.dim() != 4 or logit.shape[1] != self.ngroup * self.nclass or \
                (logit.shape[0],) + tuple(logit.shape[2:]) != (label.shape[0],) + tuple(label.shape[2:]):
            raise ValueError("CeRateLoss takes logit [n, %d, h, w] and label [n, %d, h, w]" % (self.ngroup * self.nclass, self.ngroup))
        native = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == logit.device for t in (logit, label)) and label.numel() > 0
        recording = self._recording(logit)
        if self._route(getattr(self, "route", "library")) == "fused" and native and not (recording and return_map):
            import lic360
            if not recording:
                out = lic360.ce_rate(logit, label, self.nclass, self.ngroup, return_map=return_map)
            else:
                from .autograd import CeRateFn
                out = CeRateFn.apply(logit, label)
            if getattr(self, "check_labels", True) and int(out[2].sum()):
                raise IndexError("CeRateLoss: %d labels lie outside 0 .. %d" % (int(out[2].sum()), self.nclass - 1))
            return (out[0], out[1]) + tuple(out[3:])
        return self._library(logit, label, return_map)


class _MaskConstrainFn(torch.autograd.Function):
    """identity on the tensor it is given, after masking it in place; the gradient is masked the same way"""
    @staticmethod
    def forward(ctx, x, op):
        op[x.device.index].forward(x)
        ctx.op = op
        return x

    @staticmethod
    def backward(ctx, grad_output):
        ctx.op[grad_output.device.index].backward(grad_output)
        return grad_output, None


class MaskConv2(nn.Module):
    """The training-time form of the group-causal context convolution (reference lic360_operator/MaskConstrain.py:24-39): a dense
    `conv2d` whose weight is masked by lic360.MaskConstrainOp before every forward.  Same constructor, same parameter names
    (`weight` [c_out*ngroup, c_in*ngroup, k, k], `bias`), so checkpoints interchange; the inference path evaluates the same
    function with CconvEc / CconvDc.
    route: "library" (the default) is that dense conv2d, forward and backward.  "fused" masks `weight.data` in place in the same way, then runs
    autograd.MaskConvFn: the forward is lic360_cconv_ec (the bits CconvEc returns for the same weights), the data gradient the same kernel on
    transformed operands, the weight gradient lic360_cconv_wgrad, the bias gradient a library sum.  It takes fp32 CUDA tensors, kernel_size 5 and at
    most 249 channels on either side; anything else runs on the library.  When no plan can be created for the transposed shape, only the data
    gradient runs on the library (conv2d_input); forward and weight gradient stay native.
    One visible difference: under "library" `weight.grad` carries the dense gradient at masked taps (the mask is applied to `.data` and never
    recorded); under "fused" those entries are zero.  A per-element optimiser follows the same trajectory, since masked taps are zeroed again
    before every forward; a global gradient-norm clip sees a different norm."""
    ROUTES = ("library", "fused")
    FUSED_MAX_CHANNELS = 249

    def __init__(self, ngroup, c_in, c_out, kernel_size, hidden=False, device=0, time_it=False, route="library"):
        super().__init__()
        import lic360
        if route not in self.ROUTES:
            raise ValueError("MaskConv2: unknown route %r; the routes are %s" % (route, ", ".join(repr(r) for r in self.ROUTES)))
        devs = [device] if isinstance(device, int) else list(device)
        self.ngroup, self.constrain, self.route = int(ngroup), 6 if hidden else 5, route
        self.op = {gid: lic360.MaskConstrainOp(self.constrain, ngroup, gid, time_it) for gid in devs}
        self.weight = nn.Parameter(torch.empty((c_out * ngroup, c_in * ngroup, kernel_size, kernel_size), dtype=torch.float32))
        nn.init.kaiming_normal_(self.weight)
        self.bias = nn.Parameter(torch.zeros(c_out * ngroup, dtype=torch.float32))
        self.pad = kernel_size // 2
        self._dgrad_native = None                                           # decided at the first fused forward

    def _fused(self, x):
        nout, channel, k, _ = self.weight.shape
        return self.route == "fused" and k == 5 and max(nout, channel) <= self.FUSED_MAX_CHANNELS and x.dim() == 4 and \
            all(t.is_cuda and t.dtype == torch.float32 and t.device == x.device for t in (x, self.weight, self.bias))

    def _transposed_plan(self, device):
        """is there a plan for the data gradient's shape (c_out * ngroup -> c_in * ngroup channels)?"""
        if self._dgrad_native is None:
            import lic360
            try:
                lic360._cconv_op(self.weight.shape[0], self.ngroup, self.weight.shape[1], self.constrain, device.index)
                self._dgrad_native = True
            except lic360.Lic360Error:
                self._dgrad_native = False
        return self._dgrad_native

    def forward(self, x):
        self.weight.data = _MaskConstrainFn.apply(self.weight.data, self.op)
        if getattr(self, "route", "library") == "fused" and self._fused(x):
            from .autograd import MaskConvFn
            x = x if x.is_contiguous() else x.contiguous()
            return MaskConvFn.apply(x, self.weight, self.bias, self.ngroup, self.constrain, self._transposed_plan(x.device))
        return nn.functional.conv2d(x, self.weight, self.bias, padding=self.pad)
