"""Case table of the detection head tests (tests/test_detect_cpu.py, tests/test_detect_gpu.py, tools/detect_cost.py) and the seeded
builders of their inputs.

The kernel (csrc/detect.hip) runs one workgroup of 1024 threads per image: 16-byte loads over the aligned middle of a row of N = Q * Kc
logits with a scalar head and tail, four 8-bit radix passes, a compaction with an ordered path for ties at the k-th key, a bitonic sort
padded to a power of two, a rank sort by label, one wave per class for the suppression (64 detections per lane step)."""
import torch

IOU_THR = 0.5
SIZES = ((480., 640.), (375., 500.), (333., 512.))          # (h, w) of image 0, 1, 2

# name -> (B, Q, Kc, k, kind).  With B = 3 and N odd the rows of image 1 and 2 start 4 / 12 and 8 bytes past a 16-byte boundary.
#   N: 1, 255, 256, 257, 1023, 4099, 600 * 91;  k: 1, N, 256, 257, 300, 1024 (and 100, the COCO loop's)
CASES = {
    "n1_k1": (3, 1, 1, 1, "normal"),                         # k = N = 1: rows 4 and 8 bytes off
    "n255_kN": (3, 85, 3, 255, "normal"),                    # k = N: everything is selected; rows 12 and 8 bytes off
    "n256_k256": (2, 64, 4, 256, "normal"),                  # aligned rows, the bitonic sort needs no padding
    "n257_k257": (3, 257, 1, 257, "normal"),                 # Kc = 1: one class of 257 (> 256), rows 4 and 8 bytes off
    "n1023_k300": (3, 93, 11, 300, "distinct"),
    "n1023_k1": (2, 33, 31, 1, "normal"),
    "n4099_k1024": (3, 4099, 1, 1024, "normal"),             # the largest k, every selection in the one class: 16 detections per lane
    "voc": (2, 300, 21, 300, "distinct"),                    # the VOC loop's shape
    "voc_flip": (2, 600, 21, 300, "distinct"),               # ... with the flip test-time augmentation
    "coco": (2, 300, 91, 100, "distinct"),                   # the COCO loop's shape
    "coco_flip": (2, 600, 91, 100, "normal"),                # N = 600 * 91
    "all_equal": (3, 85, 3, 100, "equal"),                   # one key: the whole selection is a tie, resolved by index
    "low8": (2, 93, 11, 300, "low8"),                        # logits that differ in their lowest 8 bits only: the last radix pass decides
    "quantised": (2, 300, 21, 300, "quantised"),             # four values: the k-th bucket holds more elements than remain to be taken
    "specials": (3, 93, 11, 300, "specials"),                # +-inf, NaN, and the k-th key inside a run of -0.0 / +0.0
    "one_class": (2, 300, 21, 300, "one_class"),             # every selection carries label 2
    "nms_pairs": (2, 40, 5, 60, "nms_pairs"),                # the 0.5015 / 0.4993 IoU pairs of criterion_cases.nms_inputs
}
DISTINCT = tuple(n for n, c in CASES.items() if c[4] == "distinct")
NO_NMS = ("n255_kN", "voc", "quantised", "n4099_k1024")      # cases that also run with do_nms = 0
# (Q, Kc, k, status): host returns of the launcher, nothing is launched
REFUSED = ((10, 3, 0, -3), (10, 3, 31, -3), (2000, 1, 1025, -2), (2 ** 20 + 1, 1, 5, -2))


def _boxes(B, Q, g):
    """Normalised cxcywh in clusters of near-duplicates (so the suppression has work to do), a few boxes hanging over the left / top
    border (the clamp at 0) and one degenerate box."""
    centres = torch.rand(B, 6, 2, generator=g) * 0.6 + 0.2
    sizes = torch.rand(B, 6, 2, generator=g) * 0.3 + 0.1
    pick = torch.randint(0, 6, (B, Q), generator=g)
    c = torch.gather(centres, 1, pick[..., None].expand(-1, -1, 2)) + 0.02 * torch.randn(B, Q, 2, generator=g)
    s = torch.gather(sizes, 1, pick[..., None].expand(-1, -1, 2)) * (1 + 0.08 * torch.randn(B, Q, 2, generator=g))
    boxes = torch.cat([c, s], -1)
    far = torch.rand(B, Q, generator=g) < 0.05
    boxes[..., 0] = torch.where(far, boxes[..., 2] * 0.3, boxes[..., 0])          # x0 = cx - w / 2 < 0
    boxes[:, Q // 2, 2:] = 0
    return boxes.contiguous()


def inputs(name):
    """-> logits [B,Q,Kc], boxes [B,Q,4], sizes [B,2] (fp32, CPU), k."""
    B, Q, Kc, k, kind = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    N = Q * Kc
    boxes = _boxes(B, Q, g)
    sizes = torch.tensor(SIZES[:B])
    if kind == "normal":
        logits = 2 * torch.randn(B, N, generator=g) - 3
    elif kind == "distinct":                                  # pairwise distinct logits AND probabilities (asserted by the tests)
        logits = torch.stack([torch.linspace(-12, 3, N)[torch.randperm(N, generator=g)] for _ in range(B)])
    elif kind == "equal":
        logits = torch.full((B, N), -1.25)
    elif kind == "low8":
        bits = 0x3F800000 + torch.randint(0, 256, (B, N), generator=g, dtype=torch.int32)
        logits = bits.view(torch.float32)
    elif kind == "quantised":
        logits = torch.randint(0, 4, (B, N), generator=g).float() * 0.5 - 2
    elif kind == "specials":
        logits = -1 - torch.rand(B, N, generator=g)
        p = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
        zeros = torch.where(torch.rand(B, 400, generator=g) < 0.5, 0.0, -0.0)      # 400 zeros of either sign around the 300th place
        logits.scatter_(1, p[:, :400], zeros)
        logits.scatter_(1, p[:, 400:403], torch.full((B, 3), float("inf")))
        logits.scatter_(1, p[:, 403:405], torch.full((B, 2), float("nan")))
        logits.scatter_(1, p[:, 405:406], (torch.full((B, 1), 0x7FC00001, dtype=torch.int32) | -0x80000000).view(torch.float32))   # -NaN
        logits.scatter_(1, p[:, 406:420], torch.full((B, 14), float("-inf")))
        logits.scatter_(1, p[:, 420:440], 3 * torch.rand(B, 20, generator=g))
    elif kind == "one_class":
        logits = (2 * torch.randn(B, Q, Kc, generator=g) - 3)
        logits[:, :, 2] += 100
    elif kind == "nms_pairs":
        logits = 2 * torch.randn(B, Q, Kc, generator=g) - 6
        quad = torch.tensor([[0., 0., 100., 100.], [33.2, 0., 133.2, 100.], [300., 0., 400., 100.], [333.4, 0., 433.4, 100.]])
        cxcywh = torch.cat([(quad[:, :2] + quad[:, 2:]) / 2, quad[:, 2:] - quad[:, :2]], 1) / 512          # a 512 x 512 frame: exact scaling
        boxes[:, 1:5] = cxcywh
        logits[:, :, 4] = -30                                 # class 4 belongs to the four boxes alone
        logits[:, 1:5, 4] = torch.tensor([3., 2., 1., 0.])
        sizes = torch.full((B, 2), 512.)
    return logits.reshape(B, Q, Kc).contiguous(), boxes, sizes, k
