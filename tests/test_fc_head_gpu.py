"""GPU tests of the native MyLSTM head (``csrc/fc_head.hip``, ``mercury_amd.ops.fc_head``).

Stage tests hold every tensor the wrappers return to an fp64 reference formed from the kernel's
OWN inputs to that stage (y from zd and W1; statistics and a2 from the kernel's y; logits from the
kernel's a2; the backward from the kernel's y, mean, rstd, a2 and, for dW1 / dz, its bf16 dy)
with ``kernel_oracles.assert_within`` at k = K = 1e-5; ``mag`` is the sum of the absolute terms
of the element's formula.  The ReLU mask is ``a2 > 0`` of the kernel's output on both sides.
The inputs are zero-mean, so E[y^2] / var is near 1.  Shapes: (2, 96, 48, 5) the smallest
training batch, three K-chunks over eight waves, classes below a tile; (17, ...) a second row
tile with one row; (33, 160, 208, 35) K != N, N not a multiple of 32, three class tiles, the
4-row-tile instantiation; (32, 256, 256, 35) the preset's geometry scaled down.
"""
import pytest
import torch

import fc_head_oracles as fo
from kernel_oracles import K, assert_within, rbf, record
from lstm_oracles import assert_vs_bf16

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(2, 96, 48, 5), (17, 96, 48, 5), (33, 160, 208, 35), (32, 256, 256, 35)]
# the 8- and 20-row-tile instantiations (B <= 128, B <= 320), each with a partial last tile
TILE_SHAPES = [(100, 64, 48, 5), (313, 64, 48, 5)]
EPS, MO = 1e-5, 0.1


def _FH():
    from mercury_amd.ops import fc_head as FH
    return FH


def _dev_case(shape, masked):
    fc1, fc2, z, d, masks = fo.case(*shape)
    t = [p.detach().to(DEV) for p in (fc1[0].weight, fc1[0].bias, fc1[1].weight, fc1[1].bias,
                                      fc2.weight, fc2.bias, fc1[1].running_mean,
                                      fc1[1].running_var)]
    m0, m1 = (m.to(DEV) for m in masks) if masked else (None, None)
    return t, z.to(DEV), d.to(DEV), m0, m1, (1 / (1 - fo.P) if masked else 1.0)


def _fwd(FH, t, z, m0, m1, scale, train):
    w1, b1, gamma, beta, w2, b2, rm, rv = t
    rm, rv, nbt = rm.clone(), rv.clone(), torch.zeros((), dtype=torch.int64, device=DEV)
    out = FH.fc_head_fwd(z, m0, m1, scale, w1, b1, gamma, beta, rm, rv, nbt, w2, b2, EPS, MO, train)
    return out, (rm, rv, nbt)


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'masks'])
@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('shape', SHAPES + TILE_SHAPES, ids=str)
def test_stages(shape, train, masked):
    FH = _FH()
    B = shape[0]
    t, z, d, m0, m1, scale = _dev_case(shape, masked)
    w1, b1, gamma, beta, w2, b2, rm0, rv0 = t
    (logits, y, mean, rstd, a2), (rm, rv, nbt) = _fwd(FH, t, z, m0, m1, scale, train)
    again, _ = _fwd(FH, t, z, m0, m1, scale, train)
    assert all(torch.equal(a, b) for a, b in zip((logits, y, mean, rstd, a2), again))
    tag = '%s %s %s' % (shape, 'train' if train else 'eval', 'masks' if masked else 'nomask')

    def chk(name, out, ref, mag):
        record('fc_head_%s %s' % (name, tag), assert_within(out, ref, mag, K, name + ' ' + tag))

    dbl = lambda *ts: [x.double() for x in ts]
    W1b, W2b, b1d, b2d, gd, bd = dbl(rbf(w1), rbf(w2), b1, b2, gamma, beta)
    k0 = m0.double() * scale if masked else torch.ones_like(z, dtype=torch.float64)
    k1 = m1.double() * scale if masked else torch.ones_like(y, dtype=torch.float64)
    zd = rbf(z * k0.float()).double()
    chk('y', y, zd @ W1b.t() + b1d, zd.abs() @ W1b.abs().t() + b1d.abs())
    yk = y.double()
    if train:
        mean_ref, mean_mag = yk.mean(0), yk.abs().mean(0)
        var, var_mag = ((yk - mean_ref) ** 2).mean(0), (yk ** 2).mean(0)
        unb = B / (B - 1)
        chk('mean', mean, mean_ref, mean_mag)
        chk('run_mean', rm, (1 - MO) * rm0.double() + MO * mean_ref,
            (1 - MO) * rm0.double().abs() + MO * mean_mag)
        chk('run_var', rv, (1 - MO) * rv0.double() + MO * unb * var,
            (1 - MO) * rv0.double() + MO * unb * var_mag)
        assert int(nbt) == 1
    else:
        mean_ref, mean_mag, var = rm0.double(), rm0.double().abs(), rv0.double()
        assert torch.equal(mean, rm0) and torch.equal(rm, rm0) and torch.equal(rv, rv0)
        assert int(nbt) == 0                                  # eval writes no buffer
    rstd_ref = (var + EPS) ** -0.5
    chk('rstd', rstd, rstd_ref, rstd_ref)
    chk('a2', a2, torch.relu(gd * (yk - mean_ref) * rstd_ref + bd) * k1,
        (gd.abs() * (yk.abs() + mean_mag) * rstd_ref + bd.abs()) * k1)
    a2k = a2.double()
    chk('logits', logits, a2k @ W2b.t() + b2d, a2k.abs() @ W2b.abs().t() + b2d.abs())

    # ---- backward, from the kernel's saved tensors
    outs = FH.fc_head_bwd(d, z, m0, m1, scale, w1, w2, gamma, y, mean, rstd, a2, train)
    assert all(torch.equal(a, b) for a, b in zip(
        outs, FH.fc_head_bwd(d, z, m0, m1, scale, w1, w2, gamma, y, mean, rstd, a2, train)))
    dz, dw1, db1, dgamma, dbeta, dw2, db2, dy = outs
    dd, mk, rk = rbf(d).double(), mean.double(), rstd.double()
    relu = (a2k > 0).double()
    dh, dh_mag = dd @ W2b * k1 * relu, dd.abs() @ W2b.abs() * k1 * relu
    xh, xh_mag = (yk - mk) * rk, (yk.abs() + mk.abs()) * rk
    dbeta_ref, dbeta_mag = dh.sum(0), dh_mag.sum(0)
    dgamma_ref, dgamma_mag = (dh * xh).sum(0), (dh_mag * xh_mag).sum(0)
    sc = gd * rk
    if train:
        dy_ref = sc * (dh - dbeta_ref / B - xh * dgamma_ref / B)
        dy_mag = sc.abs() * (dh_mag + dbeta_mag / B + xh_mag * dgamma_mag / B)
    else:
        dy_ref, dy_mag = sc * dh, sc.abs() * dh_mag
    chk('dbeta', dbeta, dbeta_ref, dbeta_mag)
    chk('dgamma', dgamma, dgamma_ref, dgamma_mag)
    chk('dy', dy, dy_ref, dy_mag)
    chk('db1', db1, dy_ref.sum(0), dy_mag.sum(0))
    dyk = dy.double()
    chk('dW1', dw1, dyk.t() @ zd, dyk.abs().t() @ zd.abs())
    chk('dz', dz, dyk @ W1b * k0, dyk.abs() @ W1b.abs() * k0)
    chk('dW2', dw2, dd.t() @ a2k, dd.abs().t() @ a2k.abs())
    chk('db2', db2, d.double().sum(0), d.double().abs().sum(0))


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_module_through_autograd_vs_fp64(shape):
    fc1, fc2, z, d, _ = fo.case(*shape)
    ref = fo.chain(fc1, fc2, z, d, None, True, torch.float64)
    tb = fo.chain(fc1, fc2, z, d, None, True, torch.bfloat16)
    got = fo.run(_FH().fc_head, fc1, fc2, z, d, None, True, DEV)
    assert_vs_bf16(got, ref, tb, 'fc_head %s' % (shape,), fo.NAMES)


def test_graph_capture_replays_bit_equal():
    FH = _FH()
    t, z, d, m0, m1, scale = _dev_case((17, 96, 48, 5), True)

    w1, b1, gamma, beta, w2, b2, rm, rv = t
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)

    def step():                      # (the running statistics move on; nothing compared reads them)
        logits, y, mean, rstd, a2 = FH.fc_head_fwd(z, m0, m1, scale, w1, b1, gamma, beta, rm, rv,
                                                   nbt, w2, b2, EPS, MO, True)
        return (logits,) + FH.fc_head_bwd(d, z, m0, m1, scale, w1, w2, gamma, y, mean, rstd, a2, True)
    eager = [x.clone() for x in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = step()
    for _ in range(2):
        for x in cap:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(cap, eager))
    assert int(nbt) == 4


def test_auto_follows_the_measured_table(monkeypatch):
    from mercury_amd.models import MyLSTM
    FH = _FH()
    models = {}
    for head in ('auto', 'torch', 'native'):
        torch.manual_seed(6)
        models[head] = MyLSTM(20, 6, hidden_dim=8, head=head).to(DEV).eval()
    x = torch.randn(5, 1, 20, 12, generator=fo.gen(7)).to(DEV)
    calls = []
    real = FH.fc_head
    monkeypatch.setattr(FH, 'fc_head', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    assert (5, 32, 6) not in FH.MEASURED_NATIVE
    with torch.no_grad():
        assert torch.equal(models['auto'](x), models['torch'](x)) and not calls
        monkeypatch.setattr(FH, 'MEASURED_NATIVE', frozenset({(5, 32, 6)}))
        assert torch.equal(models['auto'](x), models['native'](x)) and len(calls) == 2


@pytest.mark.parametrize('B,K,N,dev', [(1, 96, 48, DEV), (4, 96, 40, DEV), (4, 48, 48, DEV),
                                       (4, 96, 48, 'cpu')],
                         ids=['B=1-train', 'N%16', 'K%32', 'cpu'])
def test_refusals(B, K, N, dev, monkeypatch):
    FH = _FH()
    monkeypatch.setattr(FH, 'lib', lambda: pytest.fail('a kernel was launched'))
    fc1 = torch.nn.Sequential(torch.nn.Linear(K, N), torch.nn.BatchNorm1d(N), torch.nn.ReLU()).to(dev)
    with pytest.raises(ValueError):
        FH.fc_head(torch.randn(B, K, device=dev), fc1, torch.nn.Linear(N, 5).to(dev), 0.0, True)
