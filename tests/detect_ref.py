"""CPU restatement of the detection head (csrc/detect.hip, spe_amd.infer.detect), written apart from the package's own host path:

  select   stable descending sort of the canonical key (an order-preserving uint32 image of the fp32 logit, -0.0 as +0.0, NaN above
           +inf), so equal logits come in ascending flat index; the first k;
  decode   PostProcess's fp32 box arithmetic in torch operations (one rounding each);
  order    stable sort by label;
  suppress criterion_ref.greedy_nms_ref (fp32, torchvision's arithmetic);
  compact  survivors in front, then logit -inf, label -1, box 0, query -1."""
import numpy as np
import torch

import criterion_ref as cr


def canonical_key(logits):
    """fp32 tensor -> numpy uint32 keys of the same shape."""
    u = logits.detach().contiguous().numpy().view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = np.uint32(0xFFFFFFFF)
    return key


def select(logits, k):
    """[B,Q,Kc] -> flat indices [B,k] int64 of the k best per image, best first, equal keys by index."""
    B = logits.shape[0]
    key = canonical_key(logits.reshape(B, -1))
    order = np.argsort(np.uint32(0xFFFFFFFF) - key, axis=1, kind="stable")[:, :k]
    return torch.from_numpy(order.astype(np.int64))


def post_process_boxes(boxes, sizes):
    """PostProcess (models/conditional_detr.py) on [B,Q,4] cxcywh and sizes [B,2] (h, w) -> absolute xyxy [B,Q,4], fp32."""
    cx, cy, w, h = boxes.float().unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1).clamp(min=0)
    img_h, img_w = sizes.float().unbind(1)
    return xyxy * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]


def detect_ref(logits, boxes, sizes, k, thr, do_nms=True):
    """-> {'logit' [B,k] fp32, 'label' [B,k] int64, 'box' [B,k,4] fp32, 'query' [B,k] int32, 'count' [B] int32, 'score' [B,k]}.
    'score' is PostProcess's own value of the element: taken out of the sigmoid of the WHOLE logit tensor, because ATen's CPU sigmoid
    of a short tensor may differ from that in the last bit (its vector body and its scalar tail are two implementations)."""
    B, Q, Kc = logits.shape
    idx = select(logits, k)
    flat, prob = logits.reshape(B, -1), logits.sigmoid().reshape(B, -1)
    xyxy = post_process_boxes(boxes, sizes)
    out = {"score": torch.zeros(B, k), "logit": torch.full((B, k), float("-inf")), "label": torch.full((B, k), -1, dtype=torch.int64), "box": torch.zeros(B, k, 4),
           "query": torch.full((B, k), -1, dtype=torch.int32), "count": torch.zeros(B, dtype=torch.int32)}
    for b in range(B):
        label, query = idx[b] % Kc, idx[b] // Kc
        o = torch.from_numpy(np.argsort(label.numpy(), kind="stable"))
        label, query, lg, bx = label[o], query[o], flat[b][idx[b]][o], xyxy[b][query[o]]
        keep = cr.greedy_nms_ref(bx, label, thr) if do_nms else torch.ones(k, dtype=torch.bool)
        n = int(keep.sum())
        out["logit"][b, :n], out["label"][b, :n], out["box"][b, :n] = lg[keep], label[keep], bx[keep]
        out["query"][b, :n], out["count"][b] = query[keep].to(torch.int32), n
        out["score"][b, :n] = prob[b][idx[b]][o][keep]
    return out


def results_of(ref):
    """The reference-shaped list of a detect_ref result: per image {'scores', 'labels', 'boxes'} trimmed to the count."""
    return [{"scores": ref["score"][b, :n], "labels": ref["label"][b, :n], "boxes": ref["box"][b, :n]}
            for b, n in enumerate(ref["count"].tolist())]


def same_bits(a, b):
    """torch.equal for floats with NaN payloads: compares the bit patterns."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
