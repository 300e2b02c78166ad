"""What the executor-side tests (weight_norm, weight_std, spectral, ortho_loss, ortho_init) share: the modules behind the per-op launches, bitwise
comparisons, the two flat models as the planner tests build them, and one training step with its error measures.  Imports without a GPU."""
import numpy as np
import torch


def mods():
    from sota_imagenet_amd import item_plan, ops

    return ops, item_plan


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def np_same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def resnet50():
    from sota_imagenet_amd.models import resnet50

    return resnet50()


def bresnet50():
    from sota_imagenet_amd.models import resnet50

    return resnet50(stem_type="deep", antialias=True, attn_type="eca", norm_layer="inplaceabn", norm_act="leaky_relu")


def model(dtype, num_classes, **kw):
    from sota_imagenet_amd.models import resnet50

    return resnet50(num_classes=num_classes, dtype=dtype, **kw)


def step(m, data, target, zero=True):
    """one forward and backward in training mode on the device; returns (output, gradients by parameter name)"""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    m.train()
    if zero:
        m.zero_grad()
    out = m(data.cuda())
    CrossEntropyLoss(smoothing=0.1)(out, target.cuda()).backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def conv_names(m):
    return [k for k, p in m.named_parameters() if p.dim() == 4]


def nerr(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def l2err(got, ref):
    assert torch.isfinite(got).all()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()
