#!/usr/bin/env python3
"""The fused optimizer step (tai_step_verdict + tai_fused_step, train.py --fused_step) on the full-width TAI_gray training environment.

  python tools/fused_step_bench.py [--reps 50] [--updates 20] [--out profiles/fused_step_bench.jsonl]

Builds four TAI_gray training environments at 128 x 128, 32 clips, K = T = F = 5 -- no guard; --guard --clip_grad_norm; the same with
--fused_step; the same with --ema_decay as well -- and makes real updates on each, then
  (a) launches   HIP events, median of --reps, around tai_step_verdict + tai_fused_step over the generator's table (with the EMA: 36
                 bytes per element) and the discriminator's (28), with plain and with non-temporal loads of g, m, v, against
                 tai_grad_scale + optimizer.step() (eager torch Adam) on the unfused guarded environment's tensors; the variants
                 alternate in one process and the whole comparison is made three times (`spread_ms`: the largest distance between
                 the three medians of any variant); bytes moved over the time as a fraction of the HBM peak (8 TB/s);
  (b) updates    eager milliseconds per update of the four environments, legs A B C D repeated three times, --updates each after a
                 warm-up; `spread_ms` is the largest distance between the three legs of any environment.
One JSON line, printed and appended to --out.

  python tools/fused_step_bench.py --decay [--out profiles/fused_step_decay_bench.jsonl]

--decay: tai_fused_step_decay (train.py --weight_decay) with every weight entry flagged against tai_fused_step on the same tables and the
same scalar table, for the generator's table of TAI_gray with and without the average: one process, the variants alternating, three
rounds of medians, bytes per element and TB/s; then an eager update with --fused_step --lr_schedule cosine --warmup_updates 100
--weight_decay 1e-4 against --fused_step alone, legs alternating three times, with the leg-to-leg spread."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import _native, fused_step, grad_guard, synthetic  # noqa: E402
from video_frame_inpainting_amd.environments import create_training_environment  # noqa: E402
from grad_guard_bench import event_ms  # noqa: E402

K = T = F = 5
BATCH, SIZE = 32, 128
HBM_PEAK_GBPS = 8000.0
CLIP = 1e-3                     # far below the gradient norms of an untrained network: every update clips


def make_env(name, guard, **kw):
    torch.manual_seed(0)
    env = create_training_environment(vfi.create_model('TAI_gray'), 1, os.path.join(ROOT, 'build', 'no_checkpoints'), name,
                                      K, T, F, [SIZE, SIZE], 1.0, 0.02, 1e-4, 0.5, 64, 3, 3, [0, 0], device=torch.device('cuda:0'),
                                      guard=grad_guard.GradGuard(clip_grad_norm=CLIP, patience=1 << 30) if guard else None, **kw)
    env.K, env.T, env.F = K, T, F
    env.train()
    return env


def update_ms(env, clips, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        c = clips[(i % 2) * BATCH:(i % 2 + 1) * BATCH]
        env.train_step(c[:, :K], c[:, K + T:], c[:, K:K + T])
    torch.cuda.synchronize()
    env.sync_guard()
    return (time.perf_counter() - t0) * 1e3 / n


def fused_launcher(env, which, nt):
    """tai_step_verdict + tai_fused_step over the tables the environment's last update left on the device (its gradients are still there)."""
    fs, L = env.fused, _native.lib()
    o, w = fs._opt[which], fused_step.WHICH[which]
    tb = o.tables
    n = tb.n
    rows = tb.host[4 * n:12 * n].reshape(n, 8).copy()
    stats_base = tb.result.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    k = o.k

    def run():
        _native.check(L.tai_step_verdict(stats_base, stats_base + 8 * (n + 1), n, CLIP, w, 0, 1 << 30, fs.table_len, fs.rec.data_ptr(), stream),
                      'tai_step_verdict')
        _native.check(L.tai_fused_step(tb.rows.data_ptr(), rows.ctypes.data, n, tb.n_segments, o.scalars.data_ptr(), fs.table_len, float(k.w1),
                                       float(k.b2), float(k.w2), float(k.eps), float(k.wE), fs.rec.data_ptr(), w, nt, 0, None, stream),
                      'tai_fused_step')
    elements = int(rows[:, 6].sum())
    with_ema = int(rows[rows[:, 5] != 0, 6].sum())
    return run, 28 * elements + 8 * with_ema, elements


def decay_launchers(env, schedule, weight_decay):
    """-> ({'fused': run, 'decay': run}, bytes, elements, flagged elements): tai_fused_step and tai_fused_step_decay over the generator's
    table as the environment's last update left it, on one scheduled scalar table and a record that says "ok, step 1"."""
    fs, L = env.fused, _native.lib()
    o, tb = fs._opt['G'], fs._opt['G'].tables
    n = tb.n
    rows = tb.host[4 * n:12 * n].reshape(n, 8).copy()
    dims = {name: p.dim() for name, p in o.module.named_parameters()}
    flags = np.array([int(dims[name] >= 2) for name in o.names], np.int64)
    dev = fs.device
    flags_dev = torch.from_numpy(flags).to(dev)
    group = o.optimizer.param_groups[0]
    scalars = torch.from_numpy(np.concatenate(fused_step.scheduled_table(group['lr'], group['betas'][0], group['betas'][1], fs.table_len, schedule,
                                                                         weight_decay, fs.max_steps))).to(dev)
    rec = np.zeros(fused_step.REC_WORDS, np.int64)
    rec[fused_step.R_COEFF] = int(np.array([1.0], np.float32).view(np.uint32)[0])
    rec[fused_step.R_TPRIME] = 1
    rec = torch.from_numpy(rec).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    k = [float(x) for x in o.k]

    def fused():
        _native.check(L.tai_fused_step(tb.rows.data_ptr(), rows.ctypes.data, n, tb.n_segments, scalars.data_ptr(), fs.table_len, *k, rec.data_ptr(),
                                       0, 0, 0, None, stream), 'tai_fused_step')

    def decay():
        _native.check(L.tai_fused_step_decay(tb.rows.data_ptr(), rows.ctypes.data, flags_dev.data_ptr(), flags.ctypes.data, n, tb.n_segments,
                                             scalars.data_ptr(), fs.table_len, *k, rec.data_ptr(), 0, 0, None, stream), 'tai_fused_step_decay')
    elements = int(rows[:, 6].sum())
    with_ema = int(rows[rows[:, 5] != 0, 6].sum())
    return {'fused': fused, 'decay': decay}, 28 * elements + 8 * with_ema, elements, int(rows[flags != 0, 6].sum())


def main_decay(args):
    torch.cuda.set_device(0)
    clips = torch.from_numpy(synthetic.make_clips(2 * BATCH, K + T + F, 1, SIZE, SIZE, 1002))
    schedule, wd = fused_step.Schedule('cosine', 100), 1e-4
    envs = {'fused': make_env('fsd_fused', False, fused_step=True), 'fused_ema': make_env('fsd_ema', False, fused_step=True, ema_decay=0.999),
            'scheduled': make_env('fsd_sched', False, fused_step=True, lr_schedule=schedule, weight_decay=wd)}
    for env in envs.values():
        update_ms(env, clips, 3)
    rec = {'metric': 'fused_step_decay', 'model': 'TAI_gray 128x128', 'batch': BATCH, 'KTF': [K, T, F], 'reps': args.reps,
           'library_version': _native.lib().tai_sepconv_version(), 'hbm_peak_GBps': HBM_PEAK_GBPS,
           'flags': '--lr_schedule cosine --warmup_updates 100 --weight_decay 1e-4'}
    for name in ('fused', 'fused_ema'):
        runs, nbytes, elements, flagged = decay_launchers(envs[name], schedule, wd)
        meds = {v: [] for v in runs}
        for _ in range(3):
            for v, run in runs.items():
                meds[v].append(event_ms(run, args.reps))
        ms = {v: float(np.median(x)) for v, x in meds.items()}
        spread = max(max(x) - min(x) for x in meds.values())
        rec['launch_G_' + ('ema' if name == 'fused_ema' else 'plain')] = {
            'elements': elements, 'flagged_elements': flagged, 'bytes': nbytes, 'bytes_per_element': round(nbytes / elements, 2),
            'ms_medians': {v: [round(x, 4) for x in xs] for v, xs in meds.items()}, 'ms': {v: round(x, 4) for v, x in ms.items()},
            'spread_ms': round(spread, 4), 'TBps': {v: round(nbytes / ms[v] / 1e9, 3) for v in runs},
            'decay_minus_fused_ms': round(ms['decay'] - ms['fused'], 4),
            'decay_not_slower_by_more_than_the_spread': bool(ms['decay'] - ms['fused'] <= spread)}
    legs = {name: [] for name in ('fused', 'scheduled')}
    for _ in range(3):
        for name in legs:
            update_ms(envs[name], clips, 2)
            legs[name].append(update_ms(envs[name], clips, args.updates))
    mean = {name: float(np.mean(v)) for name, v in legs.items()}
    spread = max(max(v) - min(v) for v in legs.values())
    rec['update'] = {'updates_per_leg': args.updates, 'ms_legs': {name: [round(x, 3) for x in v] for name, v in legs.items()},
                     'ms': {name: round(v, 3) for name, v in mean.items()}, 'spread_ms': round(spread, 3),
                     'scheduled_minus_fused_ms': round(mean['scheduled'] - mean['fused'], 3),
                     'scheduled_not_slower_by_more_than_the_spread': bool(mean['scheduled'] - mean['fused'] <= spread)}
    print(json.dumps(rec), flush=True)
    out = args.out or os.path.join(ROOT, 'profiles', 'fused_step_decay_bench.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(json.dumps(rec) + '\n')


def eager_launcher(env, which):
    module, optimizer = (env.generator, env.optimizer_G) if which == 'G' else (env.discriminator, env.optimizer_D)
    grads = [p.grad for p in module.parameters() if p.grad is not None]

    def run():
        grad_guard.scale_(grads, 0.999)
        optimizer.step()
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--updates', type=int, default=20)
    ap.add_argument('--out', type=str, default=None, help='default: profiles/fused_step_bench.jsonl, with --decay profiles/fused_step_decay_bench.jsonl')
    ap.add_argument('--decay', action='store_true', help='time tai_fused_step_decay against tai_fused_step instead (see above)')
    args = ap.parse_args()
    if args.decay:
        return main_decay(args)
    args.out = args.out or os.path.join(ROOT, 'profiles', 'fused_step_bench.jsonl')
    torch.cuda.set_device(0)
    clips = torch.from_numpy(synthetic.make_clips(2 * BATCH, K + T + F, 1, SIZE, SIZE, 1002))
    envs = {'plain': make_env('fsb_plain', False), 'guard': make_env('fsb_guard', True),
            'fused': make_env('fsb_fused', True, fused_step=True), 'fused_ema': make_env('fsb_ema', True, fused_step=True, ema_decay=0.999)}
    for env in envs.values():
        update_ms(env, clips, 3)                                 # real gradients in place; MIOpen's searches done
    rec = {'metric': 'fused_step', 'model': 'TAI_gray 128x128', 'batch': BATCH, 'KTF': [K, T, F], 'reps': args.reps,
           'library_version': _native.lib().tai_sepconv_version(), 'hbm_peak_GBps': HBM_PEAK_GBPS, 'clip_grad_norm': CLIP}

    # (a) the launches
    for which in 'GD':
        variants = {'fused': fused_launcher(envs['fused_ema'], which, 0), 'fused_nt': fused_launcher(envs['fused_ema'], which, 1)}
        runs = {'fused': variants['fused'][0], 'fused_nt': variants['fused_nt'][0], 'eager': eager_launcher(envs['guard'], which)}
        nbytes, elements = variants['fused'][1], variants['fused'][2]
        meds = {name: [] for name in runs}
        for _ in range(3):
            for name, run in runs.items():
                meds[name].append(event_ms(run, args.reps))
        ms = {name: float(np.median(v)) for name, v in meds.items()}
        spread = max(max(v) - min(v) for v in meds.values())
        rec['launch_' + which] = {
            'elements': elements, 'bytes': nbytes, 'ms_medians': {name: [round(x, 4) for x in v] for name, v in meds.items()},
            'ms': {name: round(v, 4) for name, v in ms.items()}, 'spread_ms': round(spread, 4),
            'GBps': {name: round(nbytes / ms[name] / 1e6, 1) for name in ('fused', 'fused_nt')},
            'fraction_of_hbm_peak': {name: round(nbytes / ms[name] / 1e6 / HBM_PEAK_GBPS, 4) for name in ('fused', 'fused_nt')},
            'nt_faster_by_more_than_the_spread': bool(ms['fused'] - ms['fused_nt'] > spread),
            'fused_faster_than_eager_by_more_than_the_spread': bool(ms['eager'] - ms['fused'] > spread)}
    envs['fused_ema'].sync_guard()

    # (b) one eager update, four environments, A B C D three times
    legs = {name: [] for name in envs}
    for _ in range(3):
        for name, env in envs.items():
            update_ms(env, clips, 2)
            legs[name].append(update_ms(env, clips, args.updates))
    mean = {name: float(np.mean(v)) for name, v in legs.items()}
    spread = max(max(v) - min(v) for v in legs.values())
    rec['update'] = {'updates_per_leg': args.updates, 'ms_legs': {name: [round(x, 3) for x in v] for name, v in legs.items()},
                     'ms': {name: round(v, 3) for name, v in mean.items()}, 'spread_ms': round(spread, 3),
                     'fused_minus_guard_ms': round(mean['fused'] - mean['guard'], 3),
                     'fused_ema_minus_guard_ms': round(mean['fused_ema'] - mean['guard'], 3),
                     'fused_minus_plain_ms': round(mean['fused'] - mean['plain'], 3),
                     'fused_not_slower_than_guard_by_more_than_the_spread': bool(mean['fused'] - mean['guard'] <= spread),
                     'waiting_reads_fused': envs['fused'].fused.waits}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
