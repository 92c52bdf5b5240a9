"""Cost of the waveform front end (csrc/pool_wave.hip pool_wave_kernel, csrc/pool_mel.hip
pool_wave_mel_kernel).

    python bench/wave_bench.py pool [--out FILE] [--runs R] [--ns N]
    python bench/wave_bench.py step [--out FILE] [--steps K] [--warmup W] [--runs R] [--ns N]
    python bench/wave_bench.py banks

``pool``: ``bench/gtime.py`` time of one pool build of 101 x 161 log-spectrograms (n_fft 200, hop
100, 16000-sample int16 clips) at P = 320 and P = 32 (batch 32): ``pool_wave_kernel`` as the
identity, with shift + gain, and as the full recipe, with the launcher's own frame chunks and with
fixed numbers of them, beside ``pool_spec_kernel``'s identity on the same-sized planar bf16
spectrogram shard; then ``pool_wave_mel_kernel`` as the identity with ``mel=80`` (80 x 161 log-mel
pools) and ``mel=80,dct=13`` (13 x 161 MFCC pools), the first also with fixed chunk counts.  Every
call advances the pool counter.  Interleaved, ``--runs`` times.  ``--delta K [--dwin N]`` times
the two mel recipes beside themselves with ``delta=K`` rows instead, the MFCC one also with fixed
chunk counts (a count whose LDS need the launcher refuses is recorded as refused).
``--speed LO:HI`` times the linear, ``mel=80`` and ``mel=80,dct=13,delta=2`` identity pools beside
themselves with ``speed=LO:HI`` (the polyphase resampler of ``csrc/pool_wave_slot.h``), each with
the launcher's own chunk count.  ``--cmvn K`` times the ``mel=80``, ``mel=80,dct=13`` and
``mel=80,dct=13,delta=2`` identity pools beside themselves with ``cmvn=K`` (two launches:
``pool_wave_mel_kernel`` into the fp32 workspace, ``pool_cmvn_kernel`` of ``csrc/pool_cmvn.hip``
from it into the pool).  ``--reverb P --rir-taps K`` times the linear and ``mel=80,dct=13,delta=2``
identity pools beside themselves with ``reverb=P`` on a bank of 8 K-tap responses
(``pool_reverb_kernel`` of ``csrc/pool_reverb.hip`` in front), the launcher's pre-pass chunk count
and a few forced ones; ``gflop_reverb`` is the padded GEMM ``P * 2 * 16128 * (K16 + 16)`` of the
slots that drew reverb on (all of them at P = 1).

``step``: the vgg11-speech preset as ``bench.py`` builds it (a spectrogram shard, no recipe)
against the same network fed from a synthetic int16 waveform shard through the full recipe,
ms/step, interleaved, ``--runs`` times.

``banks`` (no GPU): LDS bank conflicts of the A-operand read ``lds[(f0 + lane % 16) * hop + 4 k +
lane / 16]`` for a few hops -- the worst number of lanes of a wave on one of the 64 banks, by
the bank model of ``bench/lds_swizzle_check.py`` (``worst_b32``) -- and of the mel kernel's panel
write ``(4 (lane / 16) + i) * pitch + lane % 16`` and read ``(lane % 16) * pitch + 4 k + lane / 16``
for the pitches F16 + pad and M16 + pad it could take; and of the resampler's reads: the source
panel word ``((lane0 + lane) * rq >> 16) + k`` and the table word ``p(lane) * pitch + k`` for the
pitches 32 and 33 at the rates 0.5, 0.9, 1.1 and 2; and of the reverb pre-pass's clip read
``w + pad (w >> 4)``, ``w = 16 (lane % 16) + 15 - 4 si - lane / 16``, for 0, 1 and 4 pad words per
16, and its response read ``4 si + lane / 16 + lane % 16``.
One JSON line per measurement, appended to ``--out`` and printed.
"""
from __future__ import annotations

import os
if int(os.environ.get('GPU_MAX_HW_QUEUES') or 0) < 16:   # before torch loads HIP
    os.environ['GPU_MAX_HW_QUEUES'] = '16'

import argparse
import json
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bench'))

SHIFT_GAIN = 'wave:nfft=200,hop=100,shift=1600,gain=0.8:1.2,norm=-5:4'
FULL = SHIFT_GAIN + ',noise=0.8x0.1,fmask=2x10,tmask=2x20'
L, H, W = 16000, 101, 161


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'a') as f:
            f.write(line + '\n')


def _clips(n, length, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, length, dtype=torch.int16, device=dev)
    for s0 in range(0, n, 2048):
        blk = torch.randn(min(2048, n - s0), length, device=dev, generator=g)
        out[s0:s0 + 2048] = (blk * 0.2).clamp(-1, 1).mul(32767).to(torch.int16)
    return out


def bench_pool(args):
    import torch
    from gtime import gtime
    from mercury_amd import ops
    from mercury_amd.data.augment import SpecRecipe, WaveRecipe
    from mercury_amd.ops.importance import _pool_spec, _pool_wave
    ops.lib()
    dev = 'cuda'
    Ns, B = args.ns, 32
    shard, bank = _clips(Ns, L, dev, 8), _clips(6, 60 * L, dev, 9)
    planar = torch.randn(min(Ns, 4096), 1, H, W, device=dev).bfloat16()
    labels = torch.randint(0, 30, (Ns,), device=dev)
    recipes = {'identity': WaveRecipe.parse('wave:nfft=200,hop=100,norm=-5:4'),
               'shift+gain': WaveRecipe.parse(SHIFT_GAIN), 'full': WaveRecipe.parse(FULL),
               'mel=80 identity': WaveRecipe.parse('wave:nfft=200,hop=100,norm=-5:4,mel=80'),
               'mel=80,dct=13 identity':
                   WaveRecipe.parse('wave:nfft=200,hop=100,norm=-5:4,mel=80,dct=13')}
    if args.delta:          # the mel and MFCC pools again with delta rows, and fixed chunk counts
        recipes = {k: v for k, v in recipes.items() if 'mel' in k}
        for base in ('mel=80', 'mel=80,dct=13'):
            recipes['%s,delta=%d identity' % (base, args.delta)] = WaveRecipe.parse(
                'wave:nfft=200,hop=100,norm=-5:4,%s,delta=%d,dwin=%d'
                % (base, args.delta, args.dwin))
    if args.speed:
        base = 'wave:nfft=200,hop=100,norm=-5:4'
        kinds = {'identity': base, 'mel=80 identity': base + ',mel=80',
                 'mel=80,dct=13,delta=2 identity': base + ',mel=80,dct=13,delta=2'}
        recipes = {}
        for k, v in kinds.items():
            recipes[k] = WaveRecipe.parse(v)
            recipes[(k[:-9] + ',speed=' + args.speed).lstrip(',')] = WaveRecipe.parse(
                v + ',speed=' + args.speed)
    if args.cmvn:
        recipes = {}
        for k in ('mel=80', 'mel=80,dct=13', 'mel=80,dct=13,delta=2'):
            base = 'wave:nfft=200,hop=100,norm=-5:4,' + k
            recipes[k + ' identity'] = WaveRecipe.parse(base)
            recipes['%s,cmvn=%d' % (k, args.cmvn)] = WaveRecipe.parse(
                '%s,cmvn=%d' % (base, args.cmvn))
    rir = None
    if args.reverb:
        g = torch.Generator(device=dev).manual_seed(10)
        K = args.rir_taps
        rir = torch.randn(8, K, device=dev, generator=g) * torch.exp(
            -6.9 * torch.arange(K, device=dev) / K)
        recipes = {}
        for k in ('', 'mel=80,dct=13,delta=2'):
            base = ('wave:nfft=200,hop=100,norm=-5:4,' + k).rstrip(',')
            recipes[(k + ' identity').strip()] = WaveRecipe.parse(base)
            recipes[(k + ',reverb=%g' % args.reverb).lstrip(',')] = WaveRecipe.parse(
                '%s,reverb=%r' % (base, args.reverb))
    kr = WaveRecipe.parse('wave:nfft=200,hop=100,mel=80').mel_ksteps()
    mel_macs = sum(4 * (hi - lo + 1) * 16 for lo, hi in zip(kr[::2], kr[1::2]))   # per frame
    for P in (320, 32):
        ctrl = torch.zeros(4, dtype=torch.int64, device=dev)
        pool = torch.zeros(P, H, W, 8, dtype=torch.bfloat16, device=dev)
        pl = torch.zeros(P, dtype=torch.int32, device=dev)
        pi = torch.zeros(P, dtype=torch.int32, device=dev)

        def wave(recipe, chunks):
            out = pool if not recipe.mel else torch.zeros(P, *recipe.out_hw(L), 8, device=dev,
                                                          dtype=torch.bfloat16)
            kw = dict(rir=rir, rev_chunks=chunks) if recipe.reverb else dict(chunks=chunks)

            def fn():
                _pool_wave(shard, bank if recipe.noise else None, labels, ctrl, out, pl, pi, P,
                           B, 7, True, True, None, recipe, None, **kw)
                ctrl[0:1].add_(1)
            return fn

        def spec():
            _pool_spec(planar, labels[:planar.shape[0]], ctrl, pool, pl, pi, P, B, 7, True, True,
                       None, SpecRecipe(), None)
            ctrl[0:1].add_(1)

        def tick():                     # what every variant pays beside its kernel
            ctrl[0:1].add_(1)

        variants = [('pool_spec_kernel identity', 0, spec), ('counter increment alone', 0, tick)]
        for name, r in recipes.items():
            sweep = {'full': (0, 2, 3, 4, 6, 11), 'mel=80 identity': (0, 3, 4, 6, 11)}
            if args.reverb:             # (a reverb recipe's count is the pre-pass's)
                sweep = {'reverb=%g' % args.reverb: (0, 2, 4, 8, 16)}
            elif args.speed or args.cmvn:
                sweep = {}
            elif args.delta:
                sweep = {'mel=80,dct=13,delta=%d identity' % args.delta: (0, 2, 3, 4, 6, 11)}
            for chunks in sweep.get(name, (0,)):
                variants.append(('pool_wave_%skernel %s' % ('mel_' if r.mel else '', name), chunks,
                                 wave(r, chunks)))
        for run in range(args.runs):
            for label, chunks, fn in variants:
                ctrl.zero_()
                try:
                    us = gtime(fn, reps=16)
                except ValueError as e:         # a forced chunk count the launcher refuses
                    emit({'bench': 'wave_pool', 'run': run, 'P': P, 'variant': label,
                          'chunks': chunks, 'refused': str(e)}, args.out)
                    continue
                rec = {'bench': 'wave_pool', 'run': run, 'P': P, 'Ns': Ns, 'variant': label,
                       'chunks': chunks, 'us': round(us, 3)}
                if 'wave' in label:     # the padded GEMM: 176 frames x 200 x (2 x 112) columns
                    rec['gflop'] = round(P * 2 * 176 * 200 * 2 * 112 / 1e9, 3)
                if 'reverb' in label:   # 63 tiles of 256 outputs, K16 + 16 padded taps
                    rec['gflop_reverb'] = round(P * min(1.0, args.reverb) * 2 * 16128 * (
                        (args.rir_taps + 15) // 16 * 16 + 16) / 1e9, 3)
                    rec['rir_taps'] = args.rir_taps
                if 'mel' in label:      # the K steps run per 16-band tile (+ 80 x 16 for dct)
                    rec['gflop_mel'] = round(P * 2 * 176 * (mel_macs + (
                        80 * 16 if 'dct' in label else 0)) / 1e9, 4)
                emit(rec, args.out)


def bench_step(args):
    import numpy as np
    import torch
    from bench import PRESETS, preset_data
    from mercury_amd.data.augment import WaveRecipe
    from mercury_amd.engine.native import NativeEngine
    from mercury_amd.models import build_model
    pre = PRESETS['vgg11-speech']
    hw, x, y = preset_data(pre)
    clips = _clips(args.ns, L, 'cuda', 8)
    bank = _clips(6, 4 * L, 'cuda', 9)
    yw = np.arange(args.ns) % pre['classes']

    def one(recipe):
        torch.manual_seed(1234)
        net = build_model(pre['model'], pre['classes']).to('cuda')
        eng = NativeEngine(net, 'cuda', pre['batch'], 10, optimizer='adam', lr=0.001, seed=7,
                           importance=True, world_size=1, use_graphs=True, image_hw=hw,
                           augment=recipe)
        if recipe is None:
            eng.set_shard(x, y)
        else:
            eng.set_shard(clips, yw, noise=bank)
        eng.prime()
        eng.step()
        eng.build_graphs()
        for _ in range(args.warmup):
            eng.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        m = eng.read_meters()
        eng.close()
        return ms, m['loss_sum'] / max(m['count'], 1)

    full = WaveRecipe.parse(FULL)
    res = {'spectrogram shard': [], 'wave shard': []}
    for r in range(args.runs):
        for name, recipe in (('spectrogram shard', None), ('wave shard', full)):
            ms, loss = one(recipe)
            res[name].append(ms)
            emit({'bench': 'wave_step', 'run': r, 'shard': name, 'steps': args.steps,
                  'warmup': args.warmup, 'ms_per_step': round(ms, 4),
                  'train_loss': round(loss, 4)}, args.out)
    emit({'bench': 'wave_step_summary',
          **{'median_ms %s' % k: round(float(np.median(v)), 4) for k, v in res.items()},
          **{'max_minus_min_us %s' % k: round((max(v) - min(v)) * 1e3, 2)
             for k, v in res.items()}}, args.out)


def bench_banks(args):
    from lds_swizzle_check import worst_b32
    for hop in (100, 160, 128, 16, 7, 80, 64):
        worst = max(worst_b32(lambda lane: (lane % 16) * hop + 4 * k + lane // 16)
                    for k in range(4))
        emit({'bench': 'wave_banks', 'hop': hop, 'worst_lanes_per_bank': worst}, args.out)
    for width in (112, 80, 48, 272, 128, 16):       # F16 or M16
        for pad in (0, 1, 4, 8, 12):
            pitch = width + pad
            write = max(worst_b32(lambda lane: (4 * (lane // 16) + i) * pitch + lane % 16)
                        for i in range(4))
            read = max(worst_b32(lambda lane: (lane % 16) * pitch + 4 * k + lane // 16)
                       for k in range(4))
            emit({'bench': 'mel_panel_banks', 'pitch': pitch, 'pad': pad,
                  'worst_lanes_per_bank_write': write, 'worst_lanes_per_bank_read': read}, args.out)
    # the delta stencil's read (clamp(t + d) - w0) * pitch + r, t = tb + 4 (lane / 16) + i, r =
    # lane % 16, on the feature panel, away from the clip's ends and against its last frame
    for width in (16, 48, 80, 128):
        for pad in (0, 4):
            pitch = width + pad
            worst = {}
            for name, T in (('inner', 1 << 20), ('clamped', 38)):
                worst[name] = max(
                    worst_b32(lambda lane: min(max(tb + 4 * (lane // 16) + i + d, 0), T - 1)
                              * pitch + lane % 16)
                    for tb in (21, 27) for i in range(4) for d in range(-4, 5))
            emit({'bench': 'delta_panel_banks', 'pitch': pitch, 'pad': pad,
                  'worst_lanes_per_bank_read': worst['inner'],
                  'worst_lanes_per_bank_read_clamped': worst['clamped']}, args.out)


    # the resampler's FIR (wave_stage_speed): lane reads source word i0(lane) + k and table word
    # p(lane) * pitch + k, positions one stretch word apart, that is rq / 65536 source samples
    for rate in (0.5, 0.9, 1.1, 2.0):
        rq = int(round(rate * 65536))
        src, tab = 0, {32: 0, 33: 0}
        for start in range(0, 65536, 4099):         # a few sub-sample offsets of lane 0
            for k in range(32):
                src = max(src, worst_b32(lambda lane: ((start + lane * rq) >> 16) + k))
                for pitch in tab:
                    tab[pitch] = max(tab[pitch], worst_b32(
                        lambda lane: (((start + lane * rq) & 0xffff) >> 10) * pitch + k))
        emit({'bench': 'speed_fir_banks', 'rate': rate, 'worst_lanes_per_bank_source': src,
              'worst_lanes_per_bank_table_pitch32': tab[32],
              'worst_lanes_per_bank_table_pitch33': tab[33]}, args.out)
    # the reverb pre-pass (pool_reverb_kernel): the clip panel's B read over the 16 rows of a
    # tile at `pad` pad words per 16, and the response's A read
    for pad in (0, 1, 4):
        clip = max(worst_b32(lambda lane: (lambda w: w + pad * (w >> 4))(
            16 * (lane % 16) + 16 * so + 15 - 4 * si - lane // 16))
            for so in range(4) for si in range(4))
        emit({'bench': 'reverb_panel_banks', 'pad_per_16': pad,
              'worst_lanes_per_bank_clip_read': clip}, args.out)
    emit({'bench': 'reverb_rir_banks', 'worst_lanes_per_bank_rir_read': max(
        worst_b32(lambda lane: 4 * si + lane // 16 + lane % 16) for si in range(4))}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('pool', 'step', 'banks'))
    ap.add_argument('--out', default='')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--ns', type=int, default=4096)
    ap.add_argument('--delta', type=int, default=0, choices=(0, 1, 2))
    ap.add_argument('--dwin', type=int, default=2)
    ap.add_argument('--speed', default='', help='LO:HI, pool mode: speed perturbation on / off')
    ap.add_argument('--cmvn', type=int, default=0, choices=(0, 1, 2),
                    help='pool mode: per-utterance CMVN on / off')
    ap.add_argument('--reverb', type=float, default=0.0,
                    help='pool mode: room-impulse reverberation with this probability on / off')
    ap.add_argument('--rir-taps', type=int, default=2048)
    args = ap.parse_args()
    {'pool': bench_pool, 'step': bench_step, 'banks': bench_banks}[args.mode](args)


if __name__ == '__main__':
    main()
