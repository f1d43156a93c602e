"""Vision Transformer (Dosovitskiy et al. 2021) on the mi355x op layer, for
32-pixel input (vit_cifar*) and for 224-pixel input (vit_s8).

Patches are cut from the NHWC tensor by a view and one permute copy and
embedded by a Linear(patch*patch*3, dim); a learned position embedding
[S, dim] is added. Blocks are pre-norm:

    x = x + proj(attention(qkv(LN(x))))
    x = x + fc2(act(fc1(LN(x))))

mlp_act selects the MLP. "relu" (the default, vit_cifar and vit_cifar_s) runs
fc1 and fc2 as two ops.linear calls with ReLU fused into fc1's epilogue.
"gelu" (vit_cifar_gelu, vit_cifar_s_gelu) runs the pair as one ops.mlp with
the exact GELU (csrc/mlp.hip); the parameters are the same fc1 and fc2, so a
checkpoint loads into either. The head is a final LayerNorm, the mean over
the token grid (ops.global_avg_pool on [B,h,w,dim]) and a Linear; there is no
class token, so the sequence length stays (image / patch) ** 2: 64 at the
defaults.

The forward computes exactly that, but every residual add is fused into the
LayerNorm that follows it (ops.layer_norm with a residual returns the sum
and its norm from one pass, csrc/ln.hip): a block receives the stream and
the previous block's MLP output, norm2 adds the attention output, the next
block's norm1 adds the MLP output and the final LayerNorm adds the last
one. That is 2*depth + 1 LayerNorm launches, 2*depth of them with an add;
only the position add is a plain tensor add. dim is a multiple of 32 up to
4096; dim / heads must be 32 or 64. Attention is the resident kernel of
csrc/attn.hip up to 256 tokens and the streaming kernels of
csrc/attn_flash.hip above that, up to 4096 tokens (a 64x64 grid).

vit_cifar is dim 256, 4 heads, MLP 1024; vit_cifar_s is dim 384, 6 heads,
MLP 1536. Both have depth 6 and 4-pixel patches; the _gelu names are the same
shapes with mlp_act="gelu". vit_s8 is ViT-S/8 for 224-pixel input: dim 384,
6 heads, MLP 1536 with GELU, depth 12, 8-pixel patches, 784 tokens.
"""

from __future__ import annotations

import torch
from torch import nn

from .layers import LayerNorm, Linear, MultiHeadAttention, to_model_layout
from mi355x import ops


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_dim, mlp_act="relu"):
        super().__init__()
        if mlp_act not in ("relu", "gelu"):
            raise ValueError(f"ViT: mlp_act={mlp_act!r} is neither 'relu' "
                             "nor 'gelu'")
        self.mlp_act = mlp_act
        self.norm1 = LayerNorm(dim)
        self.attn = MultiHeadAttention(dim, heads)
        self.norm2 = LayerNorm(dim)
        self.fc1 = Linear(dim, mlp_dim,
                          act="relu" if mlp_act == "relu" else None)
        self.fc2 = Linear(mlp_dim, dim)

    def forward(self, x, h=None):
        """x: the stream; h: the previous block's MLP output, not yet added
        (None in front of the first block). Returns the pair for the next
        block."""
        B, S, D = x.shape
        if h is None:
            y = self.norm1(x)
        else:
            x, y = self.norm1(x, h)
        x, y = self.norm2(x, self.attn(y))
        if self.mlp_act == "relu":
            h = self.fc2(self.fc1(y.reshape(B * S, D)))
        else:
            h = ops.mlp(y.reshape(B * S, D), self.fc1.weight, self.fc1.bias,
                        self.fc2.weight, self.fc2.bias, self.mlp_act)
        return x, h.reshape(B, S, D)


class ViT(nn.Module):
    def __init__(self, image=32, patch=4, dim=256, depth=6, heads=4,
                 mlp_dim=1024, num_classes=10, mlp_act="relu"):
        super().__init__()
        if image % patch:
            raise ValueError(f"ViT: patch={patch} does not divide "
                             f"image={image}")
        self.patch, self.grid, self.dim = patch, image // patch, dim
        self.embed = Linear(patch * patch * 3, dim)
        self.pos = nn.Parameter(torch.empty(self.grid ** 2, dim))
        nn.init.trunc_normal_(self.pos, std=0.02)
        self.blocks = nn.Sequential(*(Block(dim, heads, mlp_dim, mlp_act)
                                      for _ in range(depth)))
        self.norm = LayerNorm(dim)
        self.fc = Linear(dim, num_classes)

    def forward(self, x):
        x = to_model_layout(x)  # NCHW -> NHWC, 16-bit on GPU
        B, p, g = x.shape[0], self.patch, self.grid
        if x.shape[1:] != (g * p, g * p, 3):
            raise ValueError(f"ViT: input {tuple(x.shape[1:])} (HWC) is not "
                             f"{(g * p, g * p, 3)}")
        x = x.reshape(B, g, p, g, p, 3).permute(0, 1, 3, 2, 4, 5)
        x = self.embed(x.reshape(B * g * g, p * p * 3))
        x = x.reshape(B, g * g, self.dim) + self.pos.to(x.dtype)
        h = None
        for block in self.blocks:
            x, h = block(x, h)
        x = self.norm(x) if h is None else self.norm(x, h)[1]
        x = ops.global_avg_pool(x.reshape(B, g, g, self.dim))
        return self.fc(x)


def vit_cifar(num_classes=10, mlp_act="relu"):
    return ViT(num_classes=num_classes, mlp_act=mlp_act)


def vit_cifar_s(num_classes=10, mlp_act="relu"):
    return ViT(dim=384, heads=6, mlp_dim=1536, num_classes=num_classes,
               mlp_act=mlp_act)


def vit_s8(num_classes=1000):
    return ViT(image=224, patch=8, dim=384, depth=12, heads=6, mlp_dim=1536,
               num_classes=num_classes, mlp_act="gelu")
