"""Gradient accumulation of spe_amd.dp.GradAllReducer (accum_steps > 1) on the CPU: single process and world 2 over gloo.

A cycle is accum_steps rounds of reset() / backward / finish(); the buckets of the non-final rounds join a running sum beside
the buckets (no collective), the final round merges the sum into the bucket before its all-reduce and averages by
world * accum_steps.  The model is the small Sequential of test_dp_gloo.py: one Linear used twice in the graph, one never used."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _model(seed):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    unused = torch.nn.Linear(3, 3)                          # never receives a gradient (cf. backbone.0.body.head)
    return net, unused, list(net.parameters()) + list(unused.parameters())


def _loss(net, x):
    return net(x).pow(2).sum() + net[0](x).sum()            # the first layer is used twice in the graph


def _flat_of(red, grads):
    """The bucket images of per-parameter tensors {param: tensor}: zeros wherever nothing is given (padding, unused)."""
    out = []
    for b in red.buckets:
        f = torch.zeros_like(b["flat"])
        for p, off in b["offsets"]:
            if p in grads:
                f[off:off + p.numel()] = grads[p].flatten()
        out.append(f)
    return out


@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_single_process_cycles(K, average):
    from spe_amd.dp import GradAllReducer
    net, unused, params = _model(0)
    used = list(net.parameters())
    red = GradAllReducer(params, bucket_bytes=64, accum_steps=K, average=average)
    assert len(red.buckets) > 2 and red.accum_steps == K and red.micro == 0
    assert all((b["acc"] is None) == (K == 1) for b in red.buckets)
    g = torch.Generator().manual_seed(100)
    for cycle in range(2):
        refs = []
        for m in range(K):
            x = torch.randn(5, 8, generator=g)
            assert red.micro == m
            red.reset()
            _loss(net, x).backward()
            red.finish()
            refs.append(dict(zip(used, torch.autograd.grad(_loss(net, x), used))))
            if m < K - 1:
                assert red.micro == m + 1
                assert all(b["work"] == "local" for b in red.buckets)
                # the buckets still hold this micro-step's own gradient
                for f, want in zip((b["flat"] for b in red.buckets), _flat_of(red, refs[m])):
                    assert torch.equal(f, want), (cycle, m)
        assert red.micro == 0
        mean = {p: sum(r[p] for r in refs) / K for p in used}
        for p in used:
            got = p.grad / (1 if average else K)
            assert torch.allclose(got, mean[p], atol=1e-6), (cycle, K)
        assert all(float(p.grad.abs().max()) == 0.0 for p in unused.parameters())
        if not average:
            # before averaging: ((g0 + g1) + g2), summed on the host in that order, bit for bit
            want = _flat_of(red, refs[0])
            for r in refs[1:]:
                want = [w + f for w, f in zip(want, _flat_of(red, r))]
            for b, w in zip(red.buckets, want):
                assert torch.equal(b["flat"], w), (cycle, K)
    assert set(red._static_unused) == set(unused.parameters())
    assert red.grad_scale() == 1.0                          # no optimizer folds the averaging in
    red.remove()


def test_misuse_and_recovery():
    from spe_amd.dp import GradAllReducer
    net, unused, params = _model(1)
    red = GradAllReducer(params, bucket_bytes=64, accum_steps=2)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(5, 8, generator=g) for _ in range(4)]
    with pytest.raises(ValueError):
        red.set_accum_steps(0)
    red.reset()
    _loss(net, xs[0]).backward()
    red.finish()
    assert red.micro == 1
    with pytest.raises(RuntimeError, match="inside a cycle"):
        red.set_accum_steps(3)
    assert red.accum_steps == 2
    # a backward without re-arming the buckets still fails loudly
    with pytest.raises(RuntimeError, match="re-armed"):
        _loss(net, xs[1]).backward()
    # recovery: the half-finished cycle is dropped, the next one is complete and exact
    red.restart_cycle()
    assert red.micro == 0
    red.set_accum_steps(3)
    red.set_accum_steps(2)
    used = list(net.parameters())
    refs = []
    for x in xs[2:]:
        red.reset()
        _loss(net, x).backward()
        red.finish()
        refs.append(torch.autograd.grad(_loss(net, x), used))
    assert red.micro == 0
    for p, a, b in zip(used, *refs):
        assert torch.allclose(p.grad, (a + b) / 2, atol=1e-6)
    assert all(float(p.grad.abs().max()) == 0.0 for p in unused.parameters())
    red.remove()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from spe_amd.dp import GradAllReducer
    K = 2
    net, unused, params = _model(rank)
    used = list(net.parameters())
    red = GradAllReducer(params, bucket_bytes=64, accum_steps=K)        # broadcasts rank 0's parameters
    g = torch.Generator().manual_seed(100 + rank)                       # different data per rank and micro-step
    launched_in_backward = []
    for cycle in range(3):
        local = []
        for m in range(K):
            x = torch.randn(5, 8, generator=g)
            red.reset()
            _loss(net, x).backward()
            if m == K - 1:
                launched_in_backward.append(red._next)                  # buckets whose all-reduce started before finish()
            red.finish()
            if m < K - 1:
                assert all(b["work"] == "local" for b in red.buckets) and red.micro == m + 1
            local.append(torch.cat([r.flatten() for r in torch.autograd.grad(_loss(net, x), used)]))
        mine = sum(local)
        gathered = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        mean = sum(gathered) / (world * K)
        got = torch.cat([p.grad.flatten() for p in used])
        assert torch.allclose(got, mean, atol=1e-6), (rank, cycle)
        assert all(float(p.grad.abs().max()) == 0.0 for p in unused.parameters())
    # from the second cycle on the never-used parameters are known: every bucket of the final micro-step goes out during backward
    assert launched_in_backward[1:] == [len(red.buckets)] * 2, launched_in_backward
    out[rank] = True
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_accum2():
    world = 2
    port = _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    assert dict(out) == {0: True, 1: True}
