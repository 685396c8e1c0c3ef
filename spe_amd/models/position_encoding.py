"""Position embeddings of the (padded) patch grid - the `position_embedding` the reference attaches to the backbone
(models/position_encoding.py, built at :88-98 with N_steps = hidden_dim // 2).
  sine / v2    : PositionEmbeddingSine(normalize=True) (:21-57), one HIP launch (csrc/misc.hip: pos_sine_kernel) on the [B,h,w] padding
                 mask; no parameters, no gradient.
  learned / v3 : PositionEmbeddingLearned (:60-85), two [50, N_steps] tables gathered by one HIP launch and differentiated by another
                 (csrc/pos_learned.hip); grids of at most 50 x 50 cells."""
import math

import torch
from torch import nn

from .. import kernels as K
from .. import ops


class PositionEmbeddingSine(nn.Module):
    EPS = 1e-6

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        if scale is not None and not normalize:
            raise ValueError("normalize should be True if scale is passed")
        self.num_pos_feats, self.temperature, self.normalize = num_pos_feats, temperature, normalize
        self.scale = 2 * math.pi if scale is None else scale
        # per-feature wavelengths temperature^(2*(k//2)/n): a constant table (not part of the state dict)
        k = torch.arange(num_pos_feats, dtype=torch.float32)
        self.register_buffer("_dim_t", temperature ** (2 * torch.div(k, 2, rounding_mode="floor") / num_pos_feats),
                             persistent=False)

    @torch.no_grad()
    def forward(self, tensor_list):
        mask = tensor_list.mask
        assert mask is not None
        if self._dim_t.device != mask.device:
            self._dim_t = self._dim_t.to(mask.device)
        feats = K.pos_sine(mask, self._dim_t, self.num_pos_feats, self.scale, self.EPS, self.normalize)
        return feats.permute(0, 3, 1, 2)        # the reference's [B,d,h,w]; the transformer consumes the [B,hw,d] buffer


class PositionEmbeddingLearned(nn.Module):
    """Absolute learned embedding: pos[b, c, y, x] = col_embed[x, c] for c < num_pos_feats, row_embed[y, c - num_pos_feats] above.  The
    padding mask plays no part: padded cells get embeddings (and send gradients) like any other, every image gets the same values."""
    TABLE = K.POS_TABLE_ROWS

    def __init__(self, num_pos_feats=256):
        super().__init__()
        self.row_embed = nn.Embedding(self.TABLE, num_pos_feats)
        self.col_embed = nn.Embedding(self.TABLE, num_pos_feats)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.uniform_(self.row_embed.weight)
        nn.init.uniform_(self.col_embed.weight)

    def forward(self, tensor_list):
        x = tensor_list.tensors
        B, (h, w) = x.shape[0], x.shape[-2:]
        if h > self.TABLE or w > self.TABLE:
            raise IndexError(f"learned position embedding: a {h} x {w} grid exceeds the {self.TABLE} entries of row_embed / col_embed "
                             f"(images of at most {16 * self.TABLE} pixels a side at 16-pixel patches); use position_embedding='sine'")
        feats = ops.pos_learned(self.col_embed.weight, self.row_embed.weight, B, h, w)
        return feats.permute(0, 3, 1, 2)        # the reference's [B,d,h,w]; the transformer consumes the [B,hw,d] buffer


def build_position_encoding(args):
    n_steps = args.hidden_dim // 2
    if args.position_embedding in ("v2", "sine"):
        return PositionEmbeddingSine(n_steps, normalize=True)
    if args.position_embedding in ("v3", "learned"):
        return PositionEmbeddingLearned(n_steps)
    raise ValueError(f"not supported {args.position_embedding}")
