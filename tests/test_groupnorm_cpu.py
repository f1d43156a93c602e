"""GroupNorm on the CPU path: ops.group_norm and layers.GroupNorm against
torch.nn.GroupNorm, the domain errors, and the ResNet norm="gn" variant."""

import pytest
import torch

import mi355x.ops as ops
from mi355x.models import build_model
from mi355x.models.layers import BatchNorm2d, GroupNorm


@pytest.mark.parametrize("has_res,act", [(True, "relu"), (False, "relu"),
                                         (True, None), (False, None)])
@pytest.mark.parametrize("C,G", [(64, 32), (64, 1), (8, 8), (96, 12)])
def test_op_and_layer_match_torch_groupnorm(C, G, has_res, act):
    g = torch.Generator().manual_seed(C + G)
    x = torch.randn(3, 5, 7, C, generator=g, requires_grad=True)
    res = torch.randn(3, 5, 7, C, generator=g, requires_grad=has_res)
    dy = torch.randn(3, 5, 7, C, generator=g)
    theirs = torch.nn.GroupNorm(G, C)
    with torch.no_grad():
        theirs.weight.copy_(0.5 + torch.rand(C, generator=g))
        theirs.bias.copy_(torch.randn(C, generator=g))
    ours = GroupNorm(G, C, act=act)
    ours.load_state_dict(theirs.state_dict())       # their dict into ours
    theirs.load_state_dict(ours.state_dict())       # and back
    assert set(ours.state_dict()) == {"weight", "bias"}

    want = theirs(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    if has_res:
        want = want + res
    if act:
        want = torch.relu(want)
    leaves_t = [x, theirs.weight, theirs.bias] + ([res] if has_res else [])
    want_g = torch.autograd.grad(want, leaves_t, dy)

    got = ours(x, residual=res if has_res else None)
    leaves_o = [x, ours.weight, ours.bias] + ([res] if has_res else [])
    got_g = torch.autograd.grad(got, leaves_o, dy)
    fun = ops.group_norm(x, G, ours.weight, ours.bias,
                         res if has_res else None, act)
    assert torch.equal(fun, got)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    for a, b in zip(got_g, want_g):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("C,G,says", [
    (12, 3, "channels=12"),              # not a multiple of 8
    (64, 5, "num_groups=5"),             # does not divide
    (96, 8, "per group=12"),             # cpg not a power of two
])
def test_domain_errors_name_the_value(C, G, says):
    x, w = torch.zeros(2, 4, 4, C), torch.ones(C)
    with pytest.raises(ValueError, match=says):
        ops.group_norm(x, G, w, w)


def test_resnet18_gn_trains_and_bn_keys_are_unchanged():
    torch.manual_seed(0)
    net = build_model("resnet18_gn")
    assert not any(isinstance(m, BatchNorm2d) for m in net.modules())
    assert sum(isinstance(m, GroupNorm) for m in net.modules()) == 20
    out = net(torch.randn(2, 3, 32, 32))
    out.sum().backward()
    assert out.shape == (2, 10) and torch.isfinite(out).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in net.parameters())
    # the default build: BatchNorm2d with torchvision's key layout
    keys = set(build_model("resnet18").state_dict())
    gn_keys = set(net.state_dict())
    stats = {k for k in keys if k.rsplit(".", 1)[-1] in
             ("running_mean", "running_var", "num_batches_tracked")}
    assert len(keys) == 122 and len(stats) == 60
    assert keys - stats == gn_keys
