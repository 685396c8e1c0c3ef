"""The learned position embedding on the CPU (construction and host logic only, no kernel runs): build_model accepts --position_embedding
learned / v3 with exactly the reference's parameter names and shapes (tests/golden/pos_learned_*.pt, written by tools/gen_pos_learned_golden.py
from the reference), the error paths, and the plain-indexing restatement tests/pos_learned_ref.py that the GPU kernel tests lean on - pinned to
the reference's own `pos` tensor and to torch autograd."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pos_learned_cases as pc  # noqa: E402
import pos_learned_ref as pr  # noqa: E402

GOLD = os.path.join(HERE, "golden")


def _blob(case):
    return torch.load(os.path.join(GOLD, f"pos_learned_{case}.pt"), weights_only=False)


@pytest.mark.parametrize("flag", ["learned", "v3"])
def test_build_model_accepts_learned(flag):
    from spe_amd.models import build_model
    from spe_amd.models.position_encoding import PositionEmbeddingLearned
    blob = _blob("tiny")
    pc.register_product_backbones()
    torch.manual_seed(5)
    model = build_model(pc.make_args("tiny", flag))[0]
    assert isinstance(model.backbone[1], PositionEmbeddingLearned)
    sd = model.state_dict()
    own = {k: tuple(v.shape) for k, v in sd.items()}
    assert own == blob["param_shapes"], set(own.items()) ^ set(blob["param_shapes"].items())
    model.load_state_dict({k: torch.zeros(s) for k, s in blob["param_shapes"].items()}, strict=True)
    names = dict(model.named_parameters())
    for k in pc.TABLES:
        assert own[k] == (50, 16)
        assert k in names and names[k].requires_grad and "backbone" in k          # the backbone LR group (reference main.py:177-188)
    fresh = build_model(pc.make_args("tiny", flag))[0].state_dict()
    for k in pc.TABLES:
        assert float(fresh[k].min()) >= 0.0 and float(fresh[k].max()) < 1.0       # nn.init.uniform_
        assert float(fresh[k].std()) > 0.2
    assert not torch.equal(fresh[pc.TABLES[0]], fresh[pc.TABLES[1]])


def test_sine_model_has_no_tables():
    from spe_amd.models import build_model
    pc.register_product_backbones()
    sd = build_model(pc.make_args("tiny", "sine"))[0].state_dict()
    assert not any("row_embed" in k or "col_embed" in k for k in sd)
    assert set(sd) == set(_blob("tiny")["param_shapes"]) - set(pc.TABLES)


def test_unknown_position_embedding_is_still_refused():
    from spe_amd.models import build_model
    pc.register_product_backbones()
    with pytest.raises(ValueError, match="not supported nonsense"):
        build_model(pc.make_args("tiny", "nonsense"))


@pytest.mark.parametrize("h,w", [(4, 51), (51, 4)])
def test_grid_beyond_the_tables_raises_index_error(h, w, monkeypatch):
    from spe_amd import lib
    from spe_amd.models.position_encoding import PositionEmbeddingLearned
    from spe_amd.util.misc import NestedTensor

    def no_call(name, *a):
        raise AssertionError(f"library call {name} before the grid check")
    monkeypatch.setattr(lib, "call", no_call)
    m = PositionEmbeddingLearned(16)
    x = NestedTensor(torch.zeros(1, 32, h, w), torch.zeros(1, h, w, dtype=torch.bool))
    with pytest.raises(IndexError, match=f"{h} x {w}.*50"):
        m(x)


def test_cpu_forward_raises_library_error():
    from spe_amd import lib
    from spe_amd.models.position_encoding import PositionEmbeddingLearned
    from spe_amd.util.misc import NestedTensor
    m = PositionEmbeddingLearned(16)
    x = NestedTensor(torch.zeros(2, 32, 4, 6), torch.zeros(2, 4, 6, dtype=torch.bool))
    with pytest.raises(lib.SpeLibraryError):
        m(x)


def test_restatement_reproduces_the_reference_pos():
    """fp32 tables in, the reference's [B,d,h,w] tensor out, bit for bit (the forward is a copy)."""
    blob = _blob("tiny")
    _, (model, *_), *_ = pc.build_case("tiny")
    sd = model.state_dict()
    chk = float(sum(v.detach().double().abs().sum() for v in sd.values() if v.is_floating_point()))
    assert abs(chk - blob["sd_checksum"]) <= 1e-9 * blob["sd_checksum"], "seeded weights differ from the ones the fixture was made with"
    ref = blob["pos"]
    B, d, h, w = ref.shape
    assert (B, d, h, w) == (2, 32, 4, 6)
    row, col = sd[pc.TABLES[0]], sd[pc.TABLES[1]]
    got = pr.forward(col, row, B, h, w)
    assert got.dtype == torch.float32 and torch.equal(got.permute(0, 3, 1, 2), ref)
    assert not torch.equal(pr.forward(row, col, B, h, w).permute(0, 3, 1, 2), ref)      # the fixture tells the two tables apart


@pytest.mark.parametrize("B,h,w,npf", [(1, 1, 1, 16), (2, 4, 6, 16), (3, 7, 50, 8), (2, 50, 3, 5)])
def test_restatement_adjoint_matches_autograd(B, h, w, npf):
    g = torch.Generator().manual_seed(B + 10 * h + 100 * w + npf)
    col, row = (torch.randn(50, npf, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    gout = torch.randn(B, h, w, 2 * npf, generator=g, dtype=torch.float64)
    # the reference's composition, restated with embedding lookups (models/position_encoding.py:77-84)
    x_emb = torch.nn.functional.embedding(torch.arange(w), col)
    y_emb = torch.nn.functional.embedding(torch.arange(h), row)
    pos = torch.cat([x_emb.unsqueeze(0).expand(h, w, npf), y_emb.unsqueeze(1).expand(h, w, npf)], -1).unsqueeze(0).expand(B, h, w, 2 * npf)
    assert torch.equal(pr.forward(col.detach(), row.detach(), B, h, w), pos.detach())
    dc, dr = torch.autograd.grad((pos * gout).sum(), (col, row))
    got_c, got_r = pr.adjoint(gout, h, w)
    assert got_c.shape == got_r.shape == (50, npf)
    assert float((got_c - dc).abs().max()) <= 1e-12 * float(dc.abs().max()) and float((got_r - dr).abs().max()) <= 1e-12 * float(dr.abs().max())
    assert float(got_c[w:].abs().sum()) == 0.0 and float(got_r[h:].abs().sum()) == 0.0
    assert torch.equal(pr.adjoint(gout.view(B, h * w, 2 * npf), h, w)[0], got_c)
