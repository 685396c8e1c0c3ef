"""When a cached 16-bit operand copy may be used again (kernels._copies_state for the weight copies and stacks, kernels.cached16 for the
copies an activation carries; no GPU): records built by hand around dummy copies of CPU tensors - the rule reads addresses, version
counters, sizes and shapes, never the copies."""
import gc

import torch

from spe_amd import kernels as K


def _copies(W, second=None):
    """What weight16 would cache for W, the copies themselves empty."""
    N, Kd = W.shape
    lo = None if second is None else torch.empty((N, Kd), dtype=torch.float16 if second == K.KIND_F16 else torch.bfloat16)
    return K.WeightCopies((W,), torch.empty((N, Kd), dtype=torch.bfloat16), torch.empty((Kd, N), dtype=torch.bfloat16), lo)


def _state(c, W, kind=None):
    return K._copies_state(c, (W.data_ptr(),), tuple(W.shape), kind)


def test_fresh_then_stale_by_version_and_epoch():
    W = torch.randn(6, 10)
    c = _copies(W)
    assert c.kind is None and c.versions == (W._version,) and c.epoch == K._W16_EPOCH and c.shape == (6, 10)
    assert _state(c, W) == "current"
    W.mul_(2.0)                                  # what a torch optimizer does
    assert _state(c, W) == "version"
    c = _copies(W)
    assert _state(c, W) == "current"
    W.data.mul_(2.0)                             # what a raw-pointer update does: no version bump ...
    assert _state(c, W) == "current"
    K.weights_changed()                          # ... so its author has to say so
    assert _state(c, W) == "epoch"
    W.mul_(2.0)
    assert _state(c, W) == "epoch"               # the batched refresh is asked for first: it makes the version current as well
    assert _state(_copies(W), W) == "current"


def test_dead_owner_even_with_a_tensor_of_the_same_shape_alive():
    W = torch.randn(6, 10)
    c = _copies(W)
    del W
    gc.collect()
    W2 = torch.randn(6, 10)                      # may or may not have landed on the freed address: dead either way
    assert c.owners[0]() is None
    assert _state(c, W2) == "dead"
    assert K._copies_state(c, (W2.data_ptr(),)) == "dead"          # as the batched refresh asks


def test_owner_that_moved_its_storage_is_dead_for_the_old_address():
    W = torch.randn(6, 10)
    c, ptr = _copies(W), W.data_ptr()
    keep = W.data                                # the old block stays allocated: the new one cannot land on it
    W.data = torch.randn(6, 10)                  # e.g. a parameter moved into a flat buffer
    assert W.data_ptr() != ptr and c.owners[0]() is W
    assert K._copies_state(c, (ptr,), (6, 10)) == "dead"
    del keep


def test_view_of_a_filter_is_owned_by_its_base():
    conv = torch.randn(8, 3, 2, 2)
    c = _copies(conv.view(8, -1))                # the view itself dies here
    gc.collect()
    assert c.owners[0]() is conv
    v = conv.view(8, -1)
    assert v.data_ptr() == conv.data_ptr()       # keyed by address: every new view finds the entry
    assert _state(c, v) == "current"
    assert K._copies_state(c, (v.data_ptr(),)) != "dead"
    conv.mul_(0.5)
    assert _state(c, v) == "version"
    c = _copies(conv.view(8, -1))
    del conv, v
    gc.collect()
    assert K._copies_state(c, (0,)) == "dead"


def test_owns_first_byte_last_byte_one_past():
    W = torch.randn(6, 10)
    base, nbytes = W.data_ptr(), 6 * 10 * 4
    assert K._owns(W, base) and K._owns(W, base + nbytes - 1)
    assert not K._owns(W, base + nbytes) and not K._owns(W, base - 1)
    c = _copies(W)
    last = W.view(-1)[59:].view(1, 1)            # a weight at the owner's last element
    assert K._copies_state(c, (last.data_ptr(),), (6, 10)) == "current"
    assert K._copies_state(c, (base + nbytes,), (6, 10)) == "dead"
    e = torch.empty(0, 4)                        # an empty owner covers one element, not none: its own address is inside
    assert K._owns(e, e.data_ptr()) and not K._owns(e, e.data_ptr() + 4)


def test_kind_of_the_second_copy_and_shape():
    W = torch.randn(6, 10)
    for have in (None, K.KIND_LO, K.KIND_F16):
        c = _copies(W, have)
        assert c.kind == have
        assert _state(c, W) == "current"                           # no second copy asked for: any record serves
        for want in (K.KIND_LO, K.KIND_F16):
            assert _state(c, W, want) == ("current" if want == have else "kind")
    c = _copies(W, K.KIND_LO)
    assert K._copies_state(c, (W.data_ptr(),), (10, 6), K.KIND_LO) == "shape"
    assert K._copies_state(c, (W.data_ptr(),), (6, 10), K.KIND_LO) == "current"


def test_stack_record_follows_every_weight_and_bias():
    Ws = [torch.randn(4, 10), torch.randn(6, 10)]
    bs = [torch.randn(4), torch.randn(6)]
    ptrs, bvers = [W.data_ptr() for W in Ws], lambda: tuple(b._version for b in bs)
    mk = lambda: K.WeightCopies(Ws, None, None, torch.empty((10, 10), dtype=torch.float16), bias=torch.cat(bs), bias_versions=bvers())
    c = mk()                                     # an fp16 stack: nothing but the second copy
    assert c.kind == K.KIND_F16 and c.shape == (10, 10) and len(c.owners) == 2
    assert K._copies_state(c, ptrs, (10, 10), K.KIND_F16, bvers()) == "current"
    assert K._copies_state(c, ptrs, (10, 10), K.KIND_LO, bvers()) == "kind"
    assert K._copies_state(c, ptrs, (12, 10), K.KIND_F16, bvers()) == "shape"
    bs[1].add_(1.0)
    assert K._copies_state(c, ptrs, (10, 10), K.KIND_F16, bvers()) == "version"
    c = mk()
    Ws[1].add_(1.0)
    assert K._copies_state(c, ptrs, (10, 10), K.KIND_F16, bvers()) == "version"
    c = mk()
    Ws[0] = None
    gc.collect()
    assert K._copies_state(c, ptrs, (10, 10), K.KIND_F16, bvers()) == "dead"


def test_activation_copies():
    src = torch.randn(2, 5, 8)
    x2 = src.view(10, 8)
    assert K.cached16(x2, None) == (None, None) and K.cached16(x2, src) == (None, None)
    x16 = torch.empty((10, 8), dtype=torch.bfloat16)
    for dt, have in ((None, None), (torch.bfloat16, K.KIND_LO), (torch.float16, K.KIND_F16)):
        sec = None if dt is None else torch.empty((10, 8), dtype=dt)
        K.attach16(src, x16, sec)
        assert src._spe16.kind == have and src._spe16.version == src._version
        got = K.cached16(x2, src)
        assert got[0] is x16 and got[1] is None                    # no second copy asked for: none handed out
        for want in (K.KIND_LO, K.KIND_F16):
            got = K.cached16(x2, src, want)
            assert (got[0] is x16 and got[1] is sec) if want == have else got == (None, None)
    assert K.cached16(src.view(5, 16), src) == (None, None)        # another shape
    src.add_(1.0)
    assert K.cached16(x2, src) == (None, None)                     # written since
    K.attach16(src, x16)
    assert K.cached16(x2, src)[0] is x16
