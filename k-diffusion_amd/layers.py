"""Karras et al. preconditioned denoiser wrapper (k_diffusion/layers.py:45-111, sampling part).

``Denoiser(inner_model, sigma_data)`` keeps the reference's constructor, attributes
(``inner_model``, ``sigma_data``, ``weighting``, ``scales``) and ``forward(input, sigma, **kwargs)``.
With the native HDiT inner model the three preconditioning passes (x * c_in, F * c_out, + x * c_skip)
disappear into the patch-in / patch-out GEMMs; with a foreign inner model they run as two HIP
elementwise kernels around it.  ``Denoiser.loss`` is the reference's training objective (layers.py:76-86) on HIP kernels: with the
native inner model its backward fills the parameters' ``.grad`` through the model's reverse walk (models/vjp.py); a foreign inner model
keeps its own autograd graph.  The model's dropout applies to the loss in training mode after ``model.enable_dropout()``; without it,
training mode with a dropout rate raises (``model.eval()`` gives the dropout-free objective).  The variance and simple losses and the DCT
``scales`` weighting are out of scope.
"""
import torch
from torch import nn

from . import ops


class _PrecondIn(torch.autograd.Function):
    """x * c_in (per-sample) with its transpose, the same kernel on the gradient."""

    @staticmethod
    def forward(ctx, x, sigma, sigma_data):
        ctx.save_for_backward(sigma)
        ctx.sigma_data = sigma_data
        return ops.precond_in(x, sigma, sigma_data)

    @staticmethod
    def backward(ctx, grad):
        sigma, = ctx.saved_tensors
        return ops.precond_in(grad.contiguous(), sigma, ctx.sigma_data), None, None


class _PrecondOut(torch.autograd.Function):
    """f * c_out + x * c_skip (per-sample): the gradient goes to f scaled by c_out and to x scaled by c_skip."""

    @staticmethod
    def forward(ctx, f, x, sigma, sigma_data):
        ctx.save_for_backward(sigma)
        ctx.sigma_data = sigma_data
        return ops.precond_out(f, x, sigma, sigma_data)

    @staticmethod
    def backward(ctx, grad):
        sigma, = ctx.saved_tensors
        grad = grad.contiguous()
        gf = ops.precond_vjp(grad, ops.nat.PC_OUT, sigma, ctx.sigma_data) if ctx.needs_input_grad[0] else None
        gx = ops.precond_vjp(grad, ops.nat.PC_SKIP, sigma, ctx.sigma_data) if ctx.needs_input_grad[1] else None
        return gf, gx, None, None


class _Loss(torch.autograd.Function):
    """Per-sample losses mean((f - target)^2) * c_weight from the model output f (csrc/wgrad_f32.hip: kd_loss_f32 / kd_loss_vjp_f32);
    f is the only differentiable input."""

    @staticmethod
    def forward(ctx, f, input, noised, sigma, sigma_data, weighting, c_weight):
        f = f.contiguous()
        ctx.save_for_backward(f, input, noised, sigma, c_weight)
        ctx.sigma_data, ctx.weighting = sigma_data, weighting
        return ops.loss(f, input, noised, sigma, sigma_data, weighting, c_weight)

    @staticmethod
    def backward(ctx, grad):
        f, input, noised, sigma, c_weight = ctx.saved_tensors
        g = ops.loss_vjp(f, input, noised, sigma, ctx.sigma_data, ctx.weighting, grad.to(torch.float32).contiguous(), c_weight)
        return g, None, None, None, None, None, None


_WEIGHTINGS = {'karras': ops.nat.LW_KARRAS, 'soft-min-snr': ops.nat.LW_SOFT_MIN_SNR, 'snr': ops.nat.LW_SNR}


class Denoiser(nn.Module):
    """D(x, sigma) = F(x * c_in, sigma) * c_out + x * c_skip."""

    def __init__(self, inner_model, sigma_data=1., weighting='karras', scales=1):
        super().__init__()
        self.inner_model = inner_model
        self.sigma_data = sigma_data
        self.scales = scales
        if not callable(weighting) and weighting not in ('karras', 'soft-min-snr', 'snr'):
            raise ValueError(f'Unknown weighting type {weighting}')
        self.weighting = weighting

    def get_scalings(self, sigma):
        """(c_skip, c_out, c_in) for a sigma tensor (layers.py:70-74)."""
        var = sigma ** 2 + self.sigma_data ** 2
        return self.sigma_data ** 2 / var, sigma * self.sigma_data / var ** 0.5, 1 / var ** 0.5

    def loss(self, input, noise, sigma, **kwargs):
        """Per-sample training losses [B] (layers.py:76-86): mean((F(noised c_in, sigma) - target)^2) * c_weight with noised = input + noise
        sigma and target = (input - c_skip noised) / c_out.  Backward over any scalar of them fills ``.grad`` of the inner model's
        parameters that require grad.  input, noise, sigma and the conditioning get no gradient."""
        if self.scales != 1:
            raise NotImplementedError(f'Denoiser.loss: the DCT frequency weighting (scales={self.scales}) is not implemented; use scales=1')
        for name, t in (('input', input), ('noise', noise), ('sigma', sigma), *kwargs.items()):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise NotImplementedError(f'Denoiser.loss: gradients w.r.t. {name} are not implemented (the loss differentiates w.r.t. the '
                                          f'model parameters only); pass {name}.detach()')
        x, noise = input.contiguous(), noise.contiguous()
        B = x.shape[0]
        sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
        if callable(self.weighting):
            code, c_weight = ops.nat.LW_GIVEN, self.weighting(sigma).detach().to(device=x.device, dtype=torch.float32).reshape(B).contiguous()
        else:
            code, c_weight = _WEIGHTINGS[self.weighting], None
        noised, x_in = ops.loss_prep(x, noise, sigma, self.sigma_data)
        inner = self.inner_model
        native = getattr(inner, 'loss_forward', None)
        f = native(x_in, sigma, **kwargs) if native is not None else inner(x_in, sigma, **kwargs)
        if torch.is_grad_enabled() and f.requires_grad:
            return _Loss.apply(f, x, noised, sigma, self.sigma_data, code, c_weight)
        return ops.loss(f.contiguous(), x, noised, sigma, self.sigma_data, code, c_weight)

    def prefetch_schedule(self, x_like, sigma_table, **kwargs):
        """Solver-loop hint (see ImageTransformerDenoiserModelV2.prefetch_schedule); a no-op for foreign inner models."""
        hint = getattr(self.inner_model, 'prefetch_schedule', None)
        return hint(x_like, sigma_table, **kwargs) if hint is not None else False

    def prefetch_conditioning(self, x_like, sigma, **kwargs):
        """Solver-loop hint (see ImageTransformerDenoiserModelV2.prefetch_conditioning); a no-op for foreign inner models."""
        hint = getattr(self.inner_model, 'prefetch_conditioning', None)
        if hint is not None:
            hint(x_like, sigma, **kwargs)

    def forward(self, input, sigma, **kwargs):
        inner = self.inner_model
        fused = getattr(inner, 'forward_preconditioned', None)
        if fused is not None:
            return fused(input, sigma, self.sigma_data, **kwargs)
        if torch.is_grad_enabled() and input.requires_grad and isinstance(sigma, torch.Tensor) and sigma.requires_grad:
            raise NotImplementedError('Denoiser: gradients w.r.t. sigma through the preconditioning are not implemented (only w.r.t. the '
                                      'input); pass sigma.detach()')
        sigma = sigma.to(device=input.device, dtype=torch.float32).reshape(-1).expand(input.shape[0]).contiguous()
        x = input.contiguous()
        if not torch.is_grad_enabled():
            f = inner(ops.precond_in(x, sigma, self.sigma_data), sigma, **kwargs)
            return ops.precond_out(f.contiguous(), x, sigma, self.sigma_data)
        # a differentiable inner model keeps its graph through the wrapper (layers.py:88-90 is plain autograd in the reference)
        x_in = _PrecondIn.apply(x, sigma, self.sigma_data) if x.requires_grad else ops.precond_in(x, sigma, self.sigma_data)
        f = inner(x_in, sigma, **kwargs)
        if f.requires_grad or x.requires_grad:
            return _PrecondOut.apply(f.contiguous(), x, sigma, self.sigma_data)
        return ops.precond_out(f.contiguous(), x, sigma, self.sigma_data)


    def forward_jvp(self, input, sigma, tangent, **kwargs):
        """(D(input, sigma), J_D tangent): the forward-mode derivative of the denoiser along ``tangent``, sigma and the conditioning held
        fixed (what ``likelihood.log_likelihood`` needs).  A native inner model runs its dual pass with the preconditioning folded in; a
        foreign inner model needs a ``forward_jvp(x, sigma, x_dot, **kwargs) -> (F, F_dot)`` of its own, and the preconditioning -- linear
        in x -- goes through the same kernels as in ``forward``."""
        inner = self.inner_model
        rule = getattr(inner, 'forward_jvp', None)
        if rule is None:
            raise NotImplementedError(f'Denoiser.forward_jvp: the inner model {type(inner).__name__} has no forward_jvp rule (a forward-mode '
                                      f'JVP rule is needed for log_likelihood on the HIP path)')
        if getattr(inner, 'forward_preconditioned', None) is not None:
            return rule(input, sigma, tangent, sigma_data=self.sigma_data, **kwargs)
        sigma = sigma.to(device=input.device, dtype=torch.float32).reshape(-1).expand(input.shape[0]).contiguous()
        x, xd = input.contiguous(), tangent.contiguous()
        f, fd = rule(ops.precond_in(x, sigma, self.sigma_data), sigma, ops.precond_in(xd, sigma, self.sigma_data), **kwargs)
        return ops.precond_out(f.contiguous(), x, sigma, self.sigma_data), ops.precond_out(fd.contiguous(), xd, sigma, self.sigma_data)


    def forward_vjp(self, input, sigma, **kwargs):
        """(D(input, sigma), pullback) in the shape of ``torch.func.vjp``: ``pullback(grad_out)`` = J_D^T grad_out w.r.t. ``input``, sigma and
        the conditioning held fixed (gradient guidance: the gradient of a loss on the denoised image).  A native inner model runs its own
        ``forward_vjp`` with the preconditioning folded in; a foreign inner model needs a ``forward_vjp(x, sigma, **kwargs) -> (F, pullback)``
        of its own, and the preconditioning -- linear in x -- goes through ``ops.precond_in`` / ``precond_out`` forward and
        ``ops.precond_vjp`` backward."""
        inner = self.inner_model
        rule = getattr(inner, 'forward_vjp', None)
        if rule is None:
            raise NotImplementedError(f'Denoiser.forward_vjp: the inner model {type(inner).__name__} has no forward_vjp rule (a reverse-mode '
                                      f'VJP rule is needed for input gradients on the HIP path)')
        if getattr(inner, 'forward_preconditioned', None) is not None:
            return rule(input, sigma, sigma_data=self.sigma_data, **kwargs)
        sigma = sigma.to(device=input.device, dtype=torch.float32).reshape(-1).expand(input.shape[0]).contiguous()
        x = input.contiguous()
        f, inner_pullback = rule(ops.precond_in(x, sigma, self.sigma_data), sigma, **kwargs)

        def pullback(grad_out):
            go = grad_out.contiguous()
            g = inner_pullback(ops.precond_vjp(go, ops.nat.PC_OUT, sigma, self.sigma_data))
            return ops.precond_vjp(g.contiguous(), ops.nat.PC_IN, sigma, self.sigma_data, h=go, h_coef=ops.nat.PC_SKIP)
        return ops.precond_out(f.contiguous(), x, sigma, self.sigma_data), pullback


class DenoiserWithVariance(Denoiser):
    """What ``make_denoiser_wrapper`` returns for ``has_variance`` configs (config.py:223-224; layers.py:93-101).  The reference's class
    overrides ``loss`` only (the model's log-variance output is a training quantity): ``forward`` / ``get_scalings`` -- the sampling path --
    are ``Denoiser``'s, as here."""

    def loss(self, *args, **kwargs):
        raise NotImplementedError('DenoiserWithVariance.loss (the log-variance objective) is not implemented')


class SimpleLossDenoiser(Denoiser):
    """``loss_config == 'simple'`` (config.py:229-230; layers.py:104-111): again only ``loss`` differs in the reference."""

    def loss(self, *args, **kwargs):
        raise NotImplementedError('SimpleLossDenoiser.loss (the simple objective) is not implemented')


class FourierFeatures(nn.Module):
    """``cat[cos, sin](2 pi x W^T)`` with ``W`` a ``randn([out_features // 2, in_features]) * std`` BUFFER (k_diffusion/layers.py:285-293; the
    model's ``time_emb`` and ``aug_emb``, image_transformer_v2.py:677-680, whose state_dict entries are this buffer).  The model itself reaches
    the kernel directly (``ops.fourier_sigma`` folds ``c_noise = log(sigma) / 4`` in); this is the stand-alone module of the reference's
    surface, on the same kernel (``kd_fourier_f32``: angles in revolutions, hardware sin / cos).  ROCm tensors only, like every op here."""

    def __init__(self, in_features, out_features, std=1.):
        super().__init__()
        assert out_features % 2 == 0
        self.register_buffer('weight', torch.randn([out_features // 2, in_features]) * std)

    def forward(self, input):
        x = input.to(torch.float32)
        if x.shape[-1] != self.weight.shape[1]:
            raise ValueError(f'FourierFeatures: last dimension {x.shape[-1]} != in_features {self.weight.shape[1]}')
        return ops.fourier_features(x.contiguous(), self.weight.to(torch.float32).contiguous())
