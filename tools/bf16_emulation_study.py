"""Would the opt-in bf16 convolution mode (conv_ops.set_conv_precision('bf16')) cost accuracy?  CPU only: the CPU oracle
(oracle/tai_oracle.py) once as it is (fp32) and once with every eligible convolution fed bf16-rounded operands in float64
(tests/bf16_emulation.py), on the bench's seeded weights and clips: full-width TAI_gray 128x128 T = 5 (cfg2 seed, 2 clips),
TAI_gray T = 10 (cfg5 seed, 1 clip) and TAI_color 256x256 T = 5 (cfg4 seed, 1 clip).  Per output key: max |bf16 - fp32| relative
to the key's maximum, PSNR / SSIM of the prediction against ground truth and their deltas, and the uint8 pixels that differ.

Usage (repository root):  python tools/bf16_emulation_study.py [--out profiles/r06_bf16_emulation_study.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import video_frame_inpainting_amd as vfi  # noqa: E402
from video_frame_inpainting_amd import metrics, synthetic  # noqa: E402
from oracle import tai_oracle  # noqa: E402
from bf16_emulation import bf16_oracle  # noqa: E402

KEYS = ('pred', 'pred_forward', 'pred_backward', 'interp_net_outputs_1', 'interp_net_outputs_2')
# (name, model key, c_dim, num_block, clips, H, W, K, T, F, seed name)
CASES = (('TAI_gray 128x128 T=5, 2 clips', 'TAI_gray', 1, 5, 2, 128, 128, 5, 5, 5, 'cfg2'),
         ('TAI_gray 128x128 T=10, 1 clip', 'TAI_gray', 1, 5, 1, 128, 128, 5, 10, 5, 'cfg5'),
         ('TAI_color 256x256 T=5, 1 clip', 'TAI_color', 3, 4, 1, 256, 256, 3, 5, 3, 'cfg4'))


def case_inputs(model_key, c_dim, clips, H, W, K, T, Fn, seed):
    m = synthetic.seeded_init(vfi.create_model(model_key), 0)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    c = synthetic.make_clips(clips, K + T + Fn, c_dim, H, W, synthetic.SEEDS[seed])
    P, GT, Fo = (torch.from_numpy(x) for x in synthetic.split_clip(c, K, T, Fn))
    return m, sd, P, GT, Fo


def compare(out, ref, GT):
    """{key: max |out - ref| / max |ref|}, and the prediction's PSNR / SSIM (means over frames and clips) for both, and the uint8
    pixels of the prediction that differ"""
    rel = {k: float((out[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in KEYS}
    p_o, s_o, _ = metrics.compute_errors(out['pred'].numpy(), GT.numpy())
    p_r, s_r, _ = metrics.compute_errors(ref['pred'].numpy(), GT.numpy())
    u8 = int(np.sum(metrics.to_uint8(out['pred'].numpy()) != metrics.to_uint8(ref['pred'].numpy())))
    return rel, (float(np.mean(p_r)), float(np.mean(p_o)), float(np.max(np.abs(p_o - p_r)))), \
        (float(np.mean(s_r)), float(np.mean(s_o)), float(np.max(np.abs(s_o - s_r)))), u8, out['pred'].numel()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r06_bf16_emulation_study.txt'))
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lines = ['bf16 emulation study (tools/bf16_emulation_study.py): CPU oracle, fp32 against bf16 operands / float64 sums on every',
             'eligible convolution (C >= 16, K >= 16, k in {3, 5, 7}, stride 1, padding k // 2); seeded weights (synthetic.seeded_init, 0)',
             'and the bench seeds of the clips.  PSNR / SSIM: the prediction against ground truth, mean over frames and clips; delta =',
             'the largest per-frame |bf16 - fp32|.', '']
    for name, key, c_dim, nb, clips, H, W, K, T, Fn, seed in CASES:
        t0 = time.time()
        _, sd, P, GT, Fo = case_inputs(key, c_dim, clips, H, W, K, T, Fn, seed)
        with torch.no_grad():
            ref = tai_oracle.tai_forward(sd, c_dim, nb, 51, T, P, Fo)
            with bf16_oracle() as count:
                out = tai_oracle.tai_forward(sd, c_dim, nb, 51, T, P, Fo)
        rel, psnr, ssim, u8, n = compare(out, ref, GT)
        lines.append('%s  (%.0f s; convolutions on bf16: %d distinct shapes, %d calls; left in fp32: %s)'
                     % (name, time.time() - t0, len(set(count.taken)), len(count.taken), sorted(set(count.kept))))
        lines.append('  max |bf16 - fp32| / max |fp32|:  ' + '  '.join('%s %.2e' % (k, v) for k, v in rel.items()))
        lines.append('  PSNR fp32 %.4f dB  bf16 %.4f dB  max frame delta %.4f dB' % psnr)
        lines.append('  SSIM fp32 %.6f  bf16 %.6f  max frame delta %.2e' % ssim)
        lines.append('  uint8 prediction pixels that differ: %d of %d' % (u8, n))
        lines.append('')
        print('\n'.join(lines[-6:]), flush=True)
    worst = max(float(l.split('max frame delta ')[1].split()[0]) for l in lines if l.startswith('  PSNR'))
    lines.append('largest PSNR delta: %.4f dB (%s the 0.05 dB bound of the issue)' % (worst, 'within' if worst <= 0.05 else 'OVER'))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(lines[-1])


if __name__ == '__main__':
    main()
