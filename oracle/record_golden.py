"""Record the reference implementation's results into ``tests/golden/*.npz``.

    python oracle/record_golden.py --reference PATH_TO_REFERENCE_TREE

Run once, by hand, where a checkout of the reference project is at hand; the tests read only
the fixtures.  The reference's training modules do not import cleanly, so single classes and
methods are taken from their source with ``ast`` and executed in a namespace built here;
``pytorch_model.py`` imports as it is.  Inputs come from ``tests/refutil.py``, the same
builders the tests use.  Only arrays and strings the reference computed are stored, none of
its code.
"""
from __future__ import annotations

import argparse
import ast
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import refutil  # noqa: E402


def extract(ref, relpath, names, namespace):
    src = open(os.path.join(ref, relpath)).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body
            if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    exec(compile(ast.Module(body=keep, type_ignores=[]), relpath, 'exec'), namespace)
    return namespace


def extract_method(ref, relpath, cls, meth):
    src = open(os.path.join(ref, relpath)).read()
    for n in ast.parse(src).body:
        if isinstance(n, ast.ClassDef) and n.name == cls:
            for m in n.body:
                if isinstance(m, ast.FunctionDef) and m.name == meth:
                    return ast.get_source_segment(src, m)
    raise KeyError(meth)


def save(name, **arrays):
    os.makedirs(refutil.GOLDEN, exist_ok=True)
    path = os.path.join(refutil.GOLDEN, name + '.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%d bytes)' % (os.path.relpath(path, ROOT), os.path.getsize(path)))


def record_meters(ref):
    ns = extract(ref, 'util.py', {'Average', 'EMAverage', 'Accuracy'}, {'torch': torch})
    avg, ema, acc = ns['Average'](), ns['EMAverage'](), ns['Accuracy']()
    for v, n in refutil.METER_UPDATES:
        avg.update(v, n)
        ema.update(v)
    out, lab = refutil.meter_inputs()
    acc.update(out, lab)
    save('meters', out=out.numpy(), lab=lab.numpy(), str_average=np.array(str(avg)),
         ema_value=np.float64(ema.value), str_ema=np.array(str(ema)),
         str_accuracy=np.array(str(acc)), accuracy=np.float64(acc.accuracy))


def record_update_samples(ref):
    torch.manual_seed(0)
    net = refutil.TinyNet()
    loader = refutil.FakeLoader()
    ns = {'torch': torch, 'F': F}
    exec(extract_method(ref, 'pytorch_collab.py', 'Trainer', 'update_samples').replace(
        'def update_samples', 'def ref_update_samples', 1).replace('\n    ', '\n'), ns)
    refm = extract(ref, 'util.py', {'EMAverage'}, {'torch': torch})

    class FakeSelf:
        pass
    fs = FakeSelf()
    fs.net, fs.device, fs.train_loader = net, 'cpu', loader
    fs.should_compute_importance = True
    fs.it = iter(loader)
    fs.get_next = lambda: next(fs.it)
    arrays = refutil.state_to_arrays(net)      # before scoring moves the BN running stats
    real, torch.multinomial = torch.multinomial, refutil.top_k_draw
    try:
        ema = refm['EMAverage']()
        r = ns['ref_update_samples'](fs, ema, 0.5)
    finally:
        torch.multinomial = real
    arrays['ema_value'] = np.float64(float(ema.value))
    for i, a in enumerate(r):
        arrays['r%d' % i] = torch.as_tensor(a).numpy()
    save('update_samples', **arrays)


def record_groupwise(ref):
    ns = extract(ref, 'util.py', {'Groupwise_Sampler'},
                 {'np': np, 'torch': torch, 'F': F, 'Sampler': object})
    ds = refutil.SliceDS(100)
    torch.manual_seed(0)
    net = refutil.TinyNet()
    net.eval()
    sampler = ns['Groupwise_Sampler'](ds)
    arrays = refutil.state_to_arrays(net)
    for step, (it, bs) in enumerate(refutil.GROUPWISE_SCHEDULE):
        with torch.no_grad():
            sampler.update_importance(it, bs, net, device='cpu')
        arrays['group_index.%d' % step] = np.int64(sampler.group_index)
        arrays['cur_sample_index.%d' % step] = np.int64(sampler.cur_sample_index)
        arrays['group_indicator.%d' % step] = sampler.group_indicator.copy()
        arrays['importance.%d' % step] = sampler.importance.copy()
    save('groupwise', **arrays)


def record_models(ref):
    from mercury_amd.models import VGG, ResNet18, ResNet34, ResNet50
    spec = importlib.util.spec_from_file_location('ref_pytorch_model',
                                                  os.path.join(ref, 'pytorch_model.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    cases = {'ResNet18': (lambda: ResNet18(10), lambda: m.ResNet18(10)),
             'ResNet34': (lambda: ResNet34(10), lambda: m.ResNet34(10)),
             'ResNet50': (lambda: ResNet50(10), lambda: m.ResNet50(10)),
             'VGG11': (lambda: VGG('VGG11', 30), lambda: m.VGG('VGG11', 30))}
    for name, (ours_fn, theirs_fn) in cases.items():
        torch.manual_seed(0)
        ours = ours_fn().double()
        theirs = theirs_fn().double()
        sd = theirs.state_dict()
        keys = list(sd.keys())
        theirs.load_state_dict(ours.state_dict())
        theirs.eval()
        with torch.no_grad():
            out = theirs(refutil.interchange_input(name))
        save('interchange_' + name, keys=np.array(keys),
             shapes=np.array([','.join(str(d) for d in sd[k].shape) for k in keys]),
             out=out.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a reference checkout')
    ref = ap.parse_args().reference
    record_meters(ref)
    record_update_samples(ref)
    record_groupwise(ref)
    record_models(ref)


if __name__ == '__main__':
    main()
