"""Global-norm gradient clipping on the GPU: the norm pass (csrc/optim.hip grad_sumsq_kernel +
grad_norm_finish_kernel), the optimizer kernels' gradient scale, graph replay, the engine.

Sizes come from the launch mirror (``ops.optim.grad_norm_edge_sizes``).  Error bound of the
random case: the sum of squares carries at most ``chain + depth`` roundings (``grad_norm_plan``),
all terms non-negative, so the norm is within ``(chain + depth) * 2**-24`` relative of the fp64
norm, plus one fp32 ulp for the square root's result.

Largest observed error-to-bound ratio (MI355X): 0.025 (scale 1e3; 0.017 at scale 1e-3).  The
exact-integer norms are 0 ulp off.  Engine case: ||dp|| is within 1e-7 relative of lr * c
(bound 1e-4).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
INF = float('inf')


def _ops():
    from mercury_amd import ops
    ops.lib()
    return ops


def _sizes():
    from mercury_amd.ops import optim as O
    return O.grad_norm_edge_sizes()


def _guarded(vals):
    """``vals`` on the device with 8 NaN floats behind it: a read past n poisons the norm."""
    buf = torch.full((vals.numel() + 8,), float('nan'), device=DEV)
    buf[:vals.numel()] = vals.to(DEV)
    return buf[:vals.numel()]


def _norm(g, c):
    """(norm, coefficient) as a CPU fp32 tensor; the record starts poisoned."""
    ops = _ops()
    from mercury_amd.ops import optim as O
    mx = torch.tensor([c], dtype=torch.float32, device=DEV)
    rec = torch.full((2,), -1.0, device=DEV)
    ws = torch.full((O.GN_WS_FLOATS,), float('nan'), device=DEV)
    ops.grad_norm(g, mx, rec, ws)
    return rec.cpu()


def _coef32(c, norm):
    """torch's formula in fp32 from an fp32 norm: clamp(c / (norm + 1e-6), max=1)."""
    return torch.clamp(torch.tensor(c, dtype=torch.float32) / (norm + 1e-6), max=1.0)


def _ulps(a, b):
    def o(x):
        i = int(np.float32(x).view(np.int32))
        return -(i & 0x7fffffff) if i < 0 else i
    return abs(o(a) - o(b))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_binding_plan_equals_the_python_mirror():
    ops = _ops()
    from mercury_amd.ops import optim as O
    for n in _sizes() + [2, 7, O.GN_BLOCK_SPAN + 4, 3 * O.GN_GRID_SPAN, 25_557_032]:
        n4, tail, blocks, trips, nt, u, cap = ops.lib().grad_norm_plan(n)
        pl = O.grad_norm_plan(n)
        assert (n4, tail, blocks, trips) == (pl['n4'], pl['tail'], pl['blocks'], pl['trips']), n
        assert (nt, u, cap) == (O.GN_NT, O.GN_U, O.GN_CAP)


@pytest.mark.parametrize('n', _sizes())
def test_norm_exact_on_small_integers(n):
    gen = torch.Generator().manual_seed(11)
    vals = torch.randint(-2, 3, (n,), generator=gen)
    S = int((vals.to(torch.int64) ** 2).sum())
    assert n <= 4_300_000 and 0 <= S < 2 ** 24       # every partial sum is an exact fp32 integer
    rec = _norm(_guarded(vals.float()), 1.0)
    want = np.float32(np.sqrt(np.float64(S)))
    print('n %d: S %d, norm %r, want %r' % (n, S, float(rec[0]), float(want)))
    assert _ulps(float(rec[0]), float(want)) <= 1


@pytest.mark.parametrize('scale', [1e-3, 1e3])
def test_norm_random_within_the_derived_bound(scale):
    from mercury_amd.ops import optim as O
    worst = 0.0
    for n in _sizes():
        gen = torch.Generator().manual_seed(n % 1000 + 1)
        vals = torch.randn(n, generator=gen) * scale
        ref = float(torch.linalg.vector_norm(vals.double()))
        pl = O.grad_norm_plan(n)
        bound = (pl['chain'] + pl['depth']) * 2.0 ** -24 * ref + 2.0 ** -23 * ref
        got = float(_norm(_guarded(vals), 1.0)[0])
        ratio = abs(got - ref) / bound
        worst = max(worst, ratio)
        print('scale %g n %d: chain %d depth %d, |err| / bound = %.4f'
              % (scale, n, pl['chain'], pl['depth'], ratio))
        assert ratio <= 1.0, (n, got, ref)
    print('scale %g: largest error-to-bound ratio %.4f' % (scale, worst))


def test_coefficient_formula():
    from mercury_amd.ops import optim as O
    gen = torch.Generator().manual_seed(5)
    g = _guarded(torch.randn(O.GN_BLOCK_SPAN + 5, generator=gen))
    norm = float(_norm(g, 1.0)[0])
    for c in (0.25 * norm, 0.999 * norm, 2.0 * norm, 1e-30, INF):
        rec = _norm(g, c)
        want = _coef32(c, rec[0])
        assert _bits(rec[1:2]).item() == _bits(want.reshape(1)).item(), (c, rec, want)
        assert (float(rec[1]) < 1.0) == (c < norm)
    assert float(_norm(g, INF)[1]) == 1.0 and float(_norm(g, 2.0 * norm)[1]) == 1.0


def test_two_launches_are_bit_equal():
    n = _sizes()[-1]
    g = _guarded(torch.randn(n, generator=torch.Generator().manual_seed(9)))
    a, b = _norm(g, 0.5), _norm(g, 0.5)
    assert torch.equal(_bits(a), _bits(b))
    assert math.isfinite(float(a[0])) and 0.0 < float(a[1]) < 1.0


@pytest.mark.parametrize('delta', [0, 1])          # last element in a float4 / in the scalar tail
def test_non_finite_gradients_propagate(delta):
    from mercury_amd.ops import optim as O
    n = O.GN_BLOCK_SPAN * 3 + delta
    vals = torch.randn(n, generator=torch.Generator().manual_seed(2))
    v = vals.clone()
    v[-1] = float('nan')
    rec = _norm(_guarded(v), 1.0)
    assert math.isnan(float(rec[0])) and math.isnan(float(rec[1]))
    v[-1] = INF
    rec = _norm(_guarded(v), 1.0)
    assert float(rec[0]) == INF and float(rec[1]) == 0.0
    rec = _norm(_guarded(vals), 1.0)                # and the finite data right before the guard
    assert math.isfinite(float(rec[0]))


def test_launcher_argument_checks():
    ops = _ops()
    from mercury_amd.ops import optim as O
    buf = torch.zeros(64, device=DEV)
    mx, rec = torch.ones(1, device=DEV), torch.zeros(2, device=DEV)
    ws = torch.zeros(O.GN_WS_FLOATS, device=DEV)
    with pytest.raises(ValueError, match='16-byte'):
        ops.grad_norm(buf[1:9], mx, rec, ws)
    with pytest.raises(ValueError):
        ops.lib().grad_norm(ops.ptr(buf), 0, ops.ptr(mx), ops.ptr(rec), ops.ptr(ws), ws.numel(), 0)
    with pytest.raises(ValueError, match='workspace'):
        ops.lib().grad_norm(ops.ptr(buf), 4 * O.GN_BLOCK_SPAN, ops.ptr(mx), ops.ptr(rec),
                            ops.ptr(ws), 3, 0)
    with pytest.raises(ValueError):
        ops.grad_norm(buf.cpu(), mx, rec, ws)
    with pytest.raises(TypeError):
        ops.grad_norm(buf.double(), mx, rec, ws)


# ---------------------------------------------------------------- optimizer step
def _layout(seed=1):
    """The segment layout of test_fused_optimizer_tiles_match_torch: partial 64 x 64 tiles, a
    C % 4 != 0 conv (elementwise + transpose), a plain vector."""
    gen = torch.Generator().manual_seed(seed)
    convs = [torch.randn(80, 96, 3, 3, generator=gen) * 0.1,
             torch.randn(128, 64, 1, 1, generator=gen) * 0.1,
             torch.randn(16, 6, 3, 3, generator=gen) * 0.1]
    vec = torch.randn(10, generator=gen)
    return [w.to(DEV) for w in convs], vec.to(DEV)


def _flat_opt(convs, vec, algo, **kw):
    ops = _ops()
    segs, copies, off = [], [], 0
    for w in convs:
        k, c, r, s_ = w.shape
        krsc = torch.zeros(k, r, s_, c, dtype=torch.bfloat16, device=DEV)
        crsk = torch.zeros(c, r, s_, k, dtype=torch.bfloat16, device=DEV)
        segs.append(dict(off=off, numel=w.numel(), kind=1, K=k, R=r, S=s_, C=c, Cpad=c,
                         w_krsc=krsc, w_crsk=crsk))
        copies += [krsc, crsk]
        off += (w.numel() + 3) // 4 * 4
    segs.append(dict(off=off, numel=10, kind=0))
    opt = ops.FlatOptimizer(segs, off + 12, DEV, algo, momentum=0.9, lr=1e-2, weight_decay=0.01,
                            **kw)
    assert opt.n_fjobs > 0 and opt.n_rest > 0
    for sg, w in zip(segs, convs):
        opt.p[sg['off']:sg['off'] + w.numel()] = w.permute(0, 2, 3, 1).reshape(-1)
    opt.p[off:off + 10] = vec
    return opt, segs, copies


def _set_grad(opt, segs, gs):
    for sg, g_ in zip(segs[:-1], gs[:-1]):
        opt.g[sg['off']:sg['off'] + g_.numel()] = g_.permute(0, 2, 3, 1).reshape(-1)
    o = segs[-1]['off']
    opt.g[o:o + 10] = gs[-1]


def _same(a, b, what):
    (oa, _, ca), (ob, _, cb) = a, b
    for name in ('p', 'm', 'v'):
        assert torch.equal(_bits(getattr(oa, name)), _bits(getattr(ob, name))), (what, name)
    for i, (x, y) in enumerate(zip(ca, cb)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (what, 'bf16 copy', i)
    assert oa.g.abs().max().item() == 0 and ob.g.abs().max().item() == 0


@pytest.mark.parametrize('algo', ['adam', 'adamw', 'sgd'])
def test_clipped_step_equals_premultiplied_gradient_and_torch(algo):
    def close(a, b, rtol, atol):                 # (test_kernels_gpu.close)
        a, b = a.float(), b.float()
        err = (a - b).abs().max().item()
        scale = b.abs().max().item() + 1e-6
        assert err <= atol + rtol * scale, 'max err %g (scale %g)' % (err, scale)

    convs, vec = _layout()
    c = 10.0                                     # ||randn over 78k elements|| is about 280
    A = _flat_opt(convs, vec, algo, clip_grad_norm=c)          # clipping active
    B = _flat_opt(convs, vec, algo)                            # g multiplied beforehand
    C = _flat_opt(convs, vec, algo, clip_grad_norm=INF)        # coefficient exactly 1
    D = _flat_opt(convs, vec, algo)                            # no clipping at all
    E = _flat_opt(convs, vec, algo, clip_grad_norm=c)          # clipping, split step
    assert A[0].clip_on and C[0].clip_on and not B[0].clip_on
    mid = A[1][2]['off']                                       # a segment start
    ref = [w.clone().requires_grad_(True) for w in convs] + [vec.clone().requires_grad_(True)]
    kw = dict(lr=1e-2, weight_decay=0.01)
    topt = {'adam': lambda: torch.optim.Adam(ref, **kw),
            'adamw': lambda: torch.optim.AdamW(ref, **kw),
            'sgd': lambda: torch.optim.SGD(ref, momentum=0.9, **kw)}[algo]()
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    gen = torch.Generator().manual_seed(3)
    for t in range(3):
        gs = [torch.randn(r_.shape, generator=gen).to(DEV) for r_ in ref]
        for r_, g_ in zip(ref, gs):
            r_.grad = g_.clone()
        tnorm = float(torch.nn.utils.clip_grad_norm_(ref, c))
        assert tnorm > c
        topt.step()
        step += 1
        for o in (A, B, C, D, E):
            _set_grad(o[0], o[1], gs)
        A[0].clip()
        A[0].step(step)
        assert abs(A[0].last_grad_norm() - tnorm) <= 1e-5 * tnorm
        coef = A[0].hyper[7].clone()
        assert 0.0 < float(coef) < 1.0
        B[0].g.mul_(coef)                        # one fp32 rounding per element, then no clipping
        B[0].step(step)
        _same(A, B, 'clipped vs premultiplied, step %d' % t)
        C[0].clip()
        C[0].step(step)
        D[0].step(step)
        assert float(C[0].hyper[7]) == 1.0
        _same(C, D, 'c = inf vs no clipping, step %d' % t)
        E[0].clip()
        E[0].step(step, start=mid)
        assert E[0].g[:mid].abs().max().item() > 0            # prefix untouched so far
        E[0].step(step, end=mid)
        _same(A, E, 'split vs full step, step %d' % t)
    opt, segs, copies = A
    for i, (sg, w, r_) in enumerate(zip(segs, convs, ref)):
        k, c_, r, s_ = w.shape
        got = opt.p[sg['off']:sg['off'] + w.numel()].view(k, r, s_, c_).permute(0, 3, 1, 2)
        close(got, r_.detach(), 1e-5, 1e-6)
        close(copies[2 * i].float(), r_.detach().permute(0, 2, 3, 1), 1e-2, 1e-3)
        close(copies[2 * i + 1].float(), r_.detach().permute(1, 2, 3, 0), 1e-2, 1e-3)
    o = segs[-1]['off']
    close(opt.p[o:o + 10], ref[-1].detach(), 1e-5, 1e-6)
    # and clipping changed the step: D (unclipped) went elsewhere
    assert not torch.equal(A[0].p, D[0].p)


def test_set_clip_and_argument_errors():
    convs, vec = _layout()
    off_opt = _flat_opt(convs, vec, 'sgd')[0]
    with pytest.raises(ValueError):
        off_opt.clip()
    with pytest.raises(ValueError):
        off_opt.set_clip(1.0)
    on = _flat_opt(convs, vec, 'sgd', clip_grad_norm=2.0)[0]
    for bad in (-1.0, float('nan'), 0.0):
        with pytest.raises(ValueError):
            on.set_clip(bad)
    on.set_clip(3.0)
    assert float(on.hyper[5]) == 3.0


def test_graph_replay_reads_the_current_max_norm():
    ops = _ops()
    n = 5000
    opt = ops.FlatOptimizer([dict(off=0, numel=n, kind=0)], n, DEV, 'sgd', lr=0.5, momentum=0.9,
                            clip_grad_norm=1.0)
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(4)).to(DEV)
    step = torch.ones(1, dtype=torch.int64, device=DEV)        # t = 1: m = clipped g
    norm = float(torch.linalg.vector_norm(g0.double()))
    opt.g.copy_(g0)
    opt.clip()
    opt.step(step)                                             # warm-up, eager
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    opt.g.copy_(g0)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=cap):
        opt.clip()
        opt.step(step)
    for c in (1.0, 7.0, 4.0 * norm):
        opt.set_clip(c)
        opt.g.copy_(g0)
        graph.replay()
        torch.cuda.synchronize()
        rec = opt.hyper[6:8].cpu()
        assert abs(float(rec[0]) - norm) <= 1e-5 * norm
        want = _coef32(c, rec[0])
        assert _bits(rec[1:2]).item() == _bits(want.reshape(1)).item(), c
        assert torch.equal(_bits(opt.m), _bits(g0 * want.to(DEV))), c
        assert opt.g.abs().max().item() == 0


# ---------------------------------------------------------------- eager trainer on the device
def test_eager_trainer_clips_with_the_native_norm():
    """Trainer.train_step on a HIP device: ops.grad_norm on flat.grad, then the in-place scale.
    The native norm and torch's differ in the last bits, so the coefficient does too: the
    parameters agree to a few fp32 ulps of the update, not bit for bit."""
    import copy
    import torch.nn as nn
    import torch.nn.functional as F
    from mercury_amd.config import Config
    from mercury_amd.importance import pool as ispool
    from mercury_amd.trainer import Trainer
    from mercury_amd.utils import Accuracy, Average, EMAverage

    class Loader:
        batch_size = 8

        def __init__(self):
            g = torch.Generator().manual_seed(5)
            self.batches = [(torch.arange(i * 8, (i + 1) * 8), torch.randn(8, 16, generator=g),
                             torch.randint(0, 5, (8,), generator=g)) for i in range(3)]

        def __iter__(self):
            return iter(self.batches)

        def __len__(self):
            return len(self.batches)

    c = 0.05
    torch.manual_seed(3)
    net = nn.Linear(16, 5).to(DEV)
    ref = copy.deepcopy(net)
    t = Trainer(net, torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9), Loader(), Loader(),
                None, DEV, Config(print_every=0, eval_every=0, clip_grad_norm=c))
    before = t.flat.data.clone()
    ema = EMAverage()
    probs, data, label, _, _ = t.update_samples(ema)
    t.train_step(probs, data, label, ema, Average(), Accuracy())
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    ispool.weighted_loss(F.cross_entropy(ref(data).float(), label, reduction='none'),
                         probs).backward()
    norm = float(torch.nn.utils.clip_grad_norm_(list(ref.parameters()), c))
    ropt.step()
    assert norm > c
    want = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
    assert abs(float(t._grad_norm) - norm) <= 1e-5 * norm
    # the update has norm lr * c; forward / backward kernels on the two copies are the same
    moved = float(torch.linalg.vector_norm((t.flat.data - before).double()))
    assert abs(moved - 0.1 * c) <= 1e-4 * 0.1 * c
    assert float((t.flat.data - want).abs().max()) <= 1e-6 * 0.1 * c + 2.0 ** -23


# ---------------------------------------------------------------- engine
def _clip_engine(c, lr, **kw):
    from mercury_amd.data.datasets import synthetic_arrays
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import ResNet18
    x, y = synthetic_arrays(3000, 10, seed=5)
    torch.manual_seed(7)
    net = ResNet18(10).cuda()
    eng = NativeEngine(net, 'cuda', 32, 10, optimizer='sgd', lr=lr, momentum=0.9,
                       weight_decay=0.0, seed=3, clip_grad_norm=c, **kw)
    eng.set_shard(x, y)
    eng.prime()
    return eng


def _engine_case(**kw):
    c, lr = 1e-2, 1.0
    eng = _clip_engine(c, lr, **kw)
    try:
        assert eng.opt.clip_on
        p0 = eng.opt.p.clone()
        eng.step()                               # the first step, eager
        torch.cuda.synchronize()
        norm = eng.opt.last_grad_norm()
        assert math.isfinite(norm) and norm > c, norm
        # first SGD-momentum step: p -= lr * (g * coef), ||g * coef|| = c * norm / (norm + 1e-6)
        moved = float(torch.linalg.vector_norm((eng.opt.p - p0).double()))
        want = lr * c * norm / (norm + 1e-6)
        print('first step: grad norm %.6g, ||dp|| %.9g, lr * c %.9g, rel %.3g'
              % (norm, moved, want, abs(moved - want) / want))
        assert abs(moved - lr * c) <= 1e-4 * lr * c
        eng.build_graphs()
        norms = []
        for _ in range(3):
            eng.step()
            torch.cuda.synchronize()
            norms.append(eng.opt.last_grad_norm())
        assert all(math.isfinite(v) and v > 0 for v in norms), norms
        assert len(set(norms + [norm])) == 4, (norm, norms)
        m = eng.read_meters()
        assert all(np.isfinite(float(v)) for v in m.values()), m
        assert torch.isfinite(eng.opt.p).all()
    finally:
        eng.close()


def test_engine_first_step_moves_by_lr_times_c():
    _engine_case()


def test_engine_clip_with_forced_buckets_world1():
    import torch.distributed as dist
    from mercury_amd.config import EngineOptions
    from mercury_amd.parallel.dist import free_port
    if dist.is_initialized():
        dist.destroy_process_group()
    dist.init_process_group('nccl', init_method='tcp://127.0.0.1:%d' % free_port(), rank=0,
                            world_size=1, device_id=torch.device('cuda', 0))
    try:
        _engine_case(force_buckets=True, comm='rccl', bucket_bytes=4 << 20,
                     opts=EngineOptions(rccl_one_rank=True))
    finally:
        dist.destroy_process_group()
