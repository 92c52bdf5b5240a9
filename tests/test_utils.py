import numpy as np
import torch

from mercury_amd.utils import (Accuracy, Average, EMAverage, flatten, flatten_torch_tensor,
                               quantize_tensor, unflatten, unflatten_torch_tensor)
from refutil import METER_UPDATES, golden


def test_meters_match_reference():
    ref = golden('meters')
    rb, rm = Average(), EMAverage()
    for v, n in METER_UPDATES:
        rb.update(v, n)
        rm.update(v)
    assert str(ref['str_average']) == str(rb)
    assert abs(float(ref['ema_value']) - rm.value) < 1e-12 and str(ref['str_ema']) == str(rm)
    out, lab = torch.from_numpy(ref['out']), torch.from_numpy(ref['lab'])
    m = Accuracy()
    m.update(out, lab)
    assert str(ref['str_accuracy']) == str(m) and float(ref['accuracy']) == m.accuracy


def test_average_device_lazy():
    a = Average()
    a.update(torch.tensor(2.0), 4)
    a.update(torch.tensor(4.0), 4)
    assert abs(a.average - 3.0) < 1e-6


def test_flatten_roundtrip():
    ts = [torch.randn(3, 4), [torch.randn(5), torch.randn(2, 2, 2)]]
    flat = flatten_torch_tensor(ts)
    assert flat.numel() == 12 + 5 + 8
    back = unflatten_torch_tensor(flat, ts)
    assert torch.equal(back[0], ts[0]) and torch.equal(back[1][1], ts[1][1])
    arrs = [np.arange(6).reshape(2, 3), [np.ones(4)]]
    f = flatten(arrs)
    b = unflatten(f, arrs)
    assert (b[0] == arrs[0]).all() and (b[1][0] == 1).all()


def test_quantize_unbiased():
    torch.manual_seed(0)
    a = torch.randn(2000)
    acc = torch.zeros_like(a)
    for _ in range(400):
        q = quantize_tensor(a)
        assert set(torch.unique(q.abs()).tolist()) <= {0.0, float(a.abs().max())}
        acc += q
    assert (acc / 400 - a).abs().mean() < 0.1


def test_engine_options_from_env(monkeypatch):
    """EngineOptions: defaults, and the one A/B variable (values may contain ',' and '=')."""
    from mercury_amd.config import EngineOptions
    monkeypatch.delenv('MERCURY_ENGINE_OPTS', raising=False)
    assert EngineOptions.from_env() == EngineOptions()
    monkeypatch.setenv('MERCURY_ENGINE_OPTS',
                       'hconv=score,pgemm=0,hconv_plans=32,16,128,128=64,64,1;32,8,256,256=none,'
                       'hconv_persist_grid=96')
    o = EngineOptions.from_env()
    assert o.hconv == 'score' and o.pgemm is False and o.hconv_persist_grid == 96
    assert o.hconv_plans == '32,16,128,128=64,64,1;32,8,256,256=none'
    monkeypatch.setenv('MERCURY_ENGINE_OPTS', 'no_such_option=1')
    import pytest
    with pytest.raises(ValueError):
        EngineOptions.from_env()
