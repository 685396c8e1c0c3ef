"""The shapes of tests/test_mha_gpu.py (csrc/mha_flash.hip: spe_mha_plan / spe_mha_fwd / spe_mha_bwd), a plain restatement of the
chunk plan, and the list of code sites each shape reaches.  Pure Python: tests/test_mha_ref_cpu.py checks the coverage of the
list and the pinned chunk counts without a GPU.

A case is (B, H, Lq, Lk, dk, dv, mask_family, score_family, p_drop, nch); nch is written out by hand and has to equal what
spe_mha_plan answers.

Mask families (1 = padded key); except for the one batch of `all_padded_batch` every batch keeps an unpadded key:
  none              no mask pointer at all
  tail              the last quarter of the keys
  head              the first 40 keys (2.5 tiles): the running maximum of the first chunk starts at -inf for three steps
  tile              one interior 16-key tile
  chunk0/_mid/_last every key of that chunk of the plan (nch >= 3): its partial has m = -inf, l = 0 in the merge
  scatter           half the keys, seeded
  one_key           exactly one key left per batch, a different one in each batch
  per_batch         tail, head, scatter, ... by batch index
  all_padded_batch  batch 1 has no key left; the others use scatter
Score families (q^ k^ products, log2 domain):
  normal            seeded O(1) q and k
  ascending         the row maximum rises by 4 per key tile (alpha < 1 in every step)
  descending        falls by 4 per key tile (the maximum comes first, every later p is tiny)
  wide              scores spread over +-30
  ties              four keys of different tiles / chunks carry identical k rows that hold the row maximum"""
import random

MASKS = ("none", "tail", "head", "tile", "chunk0", "chunk_mid", "chunk_last", "scatter", "one_key", "per_batch", "all_padded_batch")
SCORES = ("normal", "ascending", "descending", "wide", "ties")
HEAD_DIMS = ((96, 48), (48, 48), (8, 8), (32, 16), (64, 64), (96, 64), (40, 24), (20, 12), (72, 40), (80, 48), (10, 6))
LQS = (1, 15, 16, 17, 33, 49, 64, 65, 200)
LKS = (1, 3, 16, 17, 63, 64, 65, 77, 128, 144, 272, 336, 515)
BHS = ((1, 1), (2, 4), (3, 5))
MHA_TARGET = 1024


def plan(B, H, Lq, Lk):
    """spe_mha_plan + mha_fill: (ntq, ntk, ch_len, nch, tiles of the last chunk)."""
    ntq, ntk = (Lq + 15) // 16, (Lk + 15) // 16
    items = B * H * ((ntq + 3) // 4)
    c = (MHA_TARGET + items - 1) // items
    c = max(1, min(c, ntk // 4))
    ln = (ntk + c - 1) // c
    return fill(Lq, Lk, (ntk + ln - 1) // ln)


def fill(Lq, Lk, nch):
    """mha_fill for a requested chunk count (the backward accepts any; the forward only the planned one)."""
    ntq, ntk = (Lq + 15) // 16, (Lk + 15) // 16
    nch = max(1, min(nch, ntk))
    ch_len = (ntk + nch - 1) // nch
    nch = (ntk + ch_len - 1) // ch_len
    return ntq, ntk, ch_len, nch, ntk - (nch - 1) * ch_len


def instance(dk, dv):
    return "t96_48" if (dk, dv) == (96, 48) else "t48_48" if (dk, dv) == (48, 48) else "generic"


def pack_path(dk, dv):
    """Which spe_attn_pack_multi kernel packs contiguous, 16-byte aligned q / k / v of these head dims."""
    return "pack_rec" if dk % 4 == 0 and dv % 4 == 0 and dk <= 64 and dv <= 64 else "pack_unit"


def sites(case):
    B, H, Lq, Lk, dk, dv, mask, score, p, nch = case
    ntq, ntk, ch_len, n, last = fill(Lq, Lk, nch)
    inst = instance(dk, dv)
    s = {inst, inst + (":nch1" if n == 1 else ":nch>1"), "mask:" + mask, "score:" + score, "BH:%dx%d" % (B, H),
         "dq_store:" + ("vector" if dk % 4 == 0 else "scalar"), "dk_store:" + ("vector" if dk % 4 == 0 else "scalar"),
         "dv_store:" + ("vector" if dv % 4 == 0 else "scalar"), "ntq%%4=%d" % (ntq % 4), "Lk%%4=%d" % (Lk % 4), pack_path(dk, dv),
         "dkdv:%d,%d" % (dk, dv), "Lq:%d" % Lq, "Lk:%d" % Lk, "p:%g" % p}
    if (dk + 15) // 16 >= 5:
        s.add("dkt>=5")
        if inst == "generic":
            s.add("generic:dkt>=5")
    if dk % 16 or dv % 16:
        s.add("dim%16")
    if dk % 8 or dv % 8:
        s.add("dim%8")
    if Lq % 16:
        s.add("ragged_q")
    if Lk % 16:
        s.add("ragged_k")
    if Lk < 16:
        s.add("Lk<16")
    if n > 1:
        s.add("mask:%s:nch>1" % mask)
        s.add("dq_slab")
        s.add("nch=cap" if n == ntk // 4 else "nch<cap")
        if last == 1:
            s.add("last_chunk_one_tile")
        if last < ch_len:
            s.add("last_chunk_short")
    else:
        s.add("nch1:many_tiles" if ntk >= 8 else "nch1:few_tiles")
    if p > 0:
        s.add("dropout")
        for t in ("dq_slab", "ragged_q", "dkdv:10,6"):
            if t in s:
                s.add("dropout:" + t)
        if Lk % 4:
            s.add("dropout:Lk%4")
    return s


# every site a case list has to reach (tests/test_mha_ref_cpu.py)
REQUIRED = ({"generic:dkt>=5", "dkt>=5", "dim%16", "dim%8", "ragged_q", "ragged_k", "Lk<16", "dq_slab", "nch=cap", "nch<cap",
             "last_chunk_one_tile", "last_chunk_short", "nch1:many_tiles", "nch1:few_tiles", "pack_rec", "pack_unit",
             "dropout:dq_slab", "dropout:ragged_q", "dropout:dkdv:10,6", "dropout:Lk%4", "p:0.1", "p:0.5", "p:0"}
            | {"%s_store:%s" % (o, k) for o in ("dq", "dk", "dv") for k in ("vector", "scalar")}
            | {"ntq%%4=%d" % r for r in range(4)} | {"Lk%%4=%d" % r for r in range(4)}
            | {i + c for i in ("t96_48", "t48_48", "generic") for c in (":nch1", ":nch>1")}
            | {"mask:" + m for m in MASKS} | {"mask:%s:nch>1" % m for m in MASKS} | {"score:" + s for s in SCORES}
            | {"dkdv:%d,%d" % d for d in HEAD_DIMS} | {"Lq:%d" % v for v in LQS} | {"Lk:%d" % v for v in LKS}
            | {"BH:%dx%d" % bh for bh in BHS})


def _cases():
    c = []
    for dk, dv in HEAD_DIMS:                                   # every head-dim pair with one chunk and with four
        c.append((1, 1, 33, 77, dk, dv, "tail", "normal", 0, 1))
        c.append((2, 4, 17, 272, dk, dv, "scatter", "normal", 0, 4))
    for Lq in LQS:                                             # query-tile edges: ntq % 4, clamped qt, ragged last tile
        c.append((1, 1, Lq, 144, 32, 16, "none", "normal", 0, 2))
    for Lk, m, n in ((1, "none", 1), (3, "none", 1), (16, "tail", 1), (17, "tail", 1), (63, "head", 1), (64, "tile", 1), (65, "tail", 1),
                     (77, "scatter", 1), (128, "tail", 2), (144, "head", 2), (272, "tile", 4), (336, "tail", 5), (515, "tail", 7)):
        c.append((1, 1, 17, Lk, 40, 24, m, "normal", 0, n))
    for m in MASKS:                                            # every mask family over four chunks (5, 5, 5, 2 tiles)
        c.append((3, 5, 33, 272, 48, 48, m, "normal", 0, 4))
    for m in ("chunk0", "chunk_mid", "chunk_last"):            # five chunks, the last of one tile
        c.append((2, 4, 17, 336, 96, 48, m, "normal", 0, 5))
    for m in ("head", "tile", "scatter", "one_key", "per_batch", "all_padded_batch"):      # and inside a single chunk
        c.append((2, 4, 17, 77, 64, 64, m, "normal", 0, 1))
    for s in SCORES[1:]:
        c.append((2, 4, 17, 272, 96, 48, "none", s, 0, 4))
        c.append((1, 1, 33, 77, 20, 12, "tail", s, 0, 1))
        c.append((1, 1, 17, 515, 48, 48, "scatter", s, 0, 7))
    for p in (0.1, 0.5):
        c.append((2, 4, 33, 272, 48, 48, "tail", "normal", p, 4))          # several chunks
        c.append((1, 1, 17, 77, 32, 16, "none", "normal", p, 1))           # Lk % 4 = 1
        c.append((2, 4, 49, 515, 96, 48, "scatter", "normal", p, 7))       # Lk % 4 = 3, several chunks, dkt = 6
        c.append((3, 5, 65, 144, 64, 64, "head", "normal", p, 2))          # ragged last query tile, ntq % 4 = 1
        c.append((2, 4, 17, 63, 10, 6, "tail", "normal", p, 1))            # scalar stores
        c.append((1, 1, 33, 272, 10, 6, "none", "normal", p, 4))
    c.append((1, 1, 16, 142, 72, 40, "tail", "normal", 0.1, 2))            # Lk % 4 = 2
    c.append((32, 32, 64, 128, 8, 8, "tail", "normal", 0, 1))              # 1024 workgroups: one chunk of eight tiles
    c.append((16, 16, 17, 515, 8, 8, "none", "normal", 0, 4))              # 256 workgroups: 4 chunks of 9, 9, 9, 6 - below the cap of 8
    c.append((3, 5, 200, 515, 96, 48, "per_batch", "normal", 0, 7))        # the largest shape
    c.append((3, 5, 17, 515, 96, 64, "one_key", "normal", 0, 7))
    c.append((1, 1, 1, 3, 8, 8, "one_key", "normal", 0, 1))
    c.append((1, 1, 33, 272, 10, 6, "chunk_mid", "wide", 0, 4))
    return c


GPU_CASES = _cases()


def case_id(case):
    B, H, Lq, Lk, dk, dv, mask, score, p, nch = case
    return "b%dh%d-q%d-k%d-d%dx%d-%s-%s-p%g-c%d" % (B, H, Lq, Lk, dk, dv, mask, score, p, nch)


def _family_row(fam, b, case):
    B, H, Lq, Lk, dk, dv, _, _, _, nch = case
    ntq, ntk, ch_len, n, last = fill(Lq, Lk, nch)
    row = [0] * Lk
    if fam == "tail":
        for k in range(max(1, (3 * Lk) // 4), Lk):
            row[k] = 1
    elif fam == "head":
        assert Lk > 40
        for k in range(40):
            row[k] = 1
    elif fam == "tile":
        assert ntk >= 3
        t = ntk // 2
        for k in range(16 * t, min(16 * t + 16, Lk)):
            row[k] = 1
    elif fam in ("chunk0", "chunk_mid", "chunk_last"):
        assert n >= 3
        ch = {"chunk0": 0, "chunk_mid": n // 2, "chunk_last": n - 1}[fam]
        for k in range(16 * ch_len * ch, min(16 * ch_len * (ch + 1), Lk)):
            row[k] = 1
    elif fam == "scatter":
        rng = random.Random(1000 * Lk + 10 * b + dk)
        row = [rng.randrange(2) for _ in range(Lk)]
        row[rng.randrange(Lk)] = 0
    elif fam == "one_key":
        row = [1] * Lk
        row[one_key(case, b)] = 0
    elif fam == "all":
        row = [1] * Lk
    else:
        assert fam == "none", fam
    return row


def one_key(case, b):
    """The key batch b keeps under the one_key family."""
    return (2 + 37 * b) % case[3]


ALL_PADDED_BATCH = 1
PER_BATCH = ("tail", "head", "scatter", "tile", "none")


def mask_rows(case):
    """None or B lists of Lk flags (1 = padded key)."""
    B, fam = case[0], case[6]
    if fam == "none":
        return None
    if fam == "per_batch":
        return [_family_row(PER_BATCH[b % len(PER_BATCH)], b, case) for b in range(B)]
    if fam == "all_padded_batch":
        assert B > ALL_PADDED_BATCH
        return [_family_row("all" if b == ALL_PADDED_BATCH else "scatter", b, case) for b in range(B)]
    return [_family_row(fam, b, case) for b in range(B)]


def tie_keys(Lk):
    """Keys that share the row maximum under the `ties` family."""
    return sorted({1 % Lk, Lk // 3, Lk // 2 + 1, Lk - 1})
