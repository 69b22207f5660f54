"""Training-time validation without a GPU: which legs run for which flags, the best-snapshot rule, the CPU route of
metrics.compute_errors_device, and parallel.gather_rows across 2 and 3 gloo ranks with uneven shards."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from video_frame_inpainting_amd import metrics, parallel, synthetic, validation
from video_frame_inpainting_amd.options import TrainOptions

BASE = ['--K', '5', '--T', '3', '--F', '4', '--model_key', 'TAI_gray']


def _opt(extra):
    return TrainOptions().parse(BASE + extra, require_gpu=False)


def test_new_flag_parses_and_defaults_off():
    assert _opt([]).val_synthetic == 0
    assert _opt(['--val_synthetic', '7']).val_synthetic == 7


def test_no_validation_source_means_no_leg():
    assert validation.validation_legs(_opt([])) == []
    assert validation.validation_legs(_opt(['--alt_T', '2', '--alt_K', '1', '--alt_F', '1'])) == []
    assert not validation.Validator(_opt([]))


def test_legs_follow_their_sources_and_alt_values():
    legs = validation.validation_legs(_opt(['--val_video_list_path', 'a.txt']))
    assert [(l.name, l.K, l.T, l.F, l.source) for l in legs] == [('T', 5, 3, 4, 'a.txt')]
    # an alt list without its alt values does not run; with them it does
    legs = validation.validation_legs(_opt(['--val_video_list_path', 'a.txt', '--val_video_list_alt_T_path', 'b.txt',
                                            '--val_video_list_alt_K_F_path', 'c.txt', '--alt_K', '2']))
    assert [l.name for l in legs] == ['T']
    legs = validation.validation_legs(_opt(['--val_video_list_path', 'a.txt', '--val_video_list_alt_T_path', 'b.txt',
                                            '--val_video_list_alt_K_F_path', 'c.txt', '--alt_T', '7', '--alt_K', '2',
                                            '--alt_F', '1']))
    assert [(l.name, l.K, l.T, l.F, l.source) for l in legs] == [('T', 5, 3, 4, 'a.txt'), ('altT', 5, 7, 4, 'b.txt'),
                                                                 ('altKF', 2, 3, 1, 'c.txt')]
    # only the alt-T list: that leg alone
    legs = validation.validation_legs(_opt(['--val_video_list_alt_T_path', 'b.txt', '--alt_T', '7']))
    assert [l.name for l in legs] == ['altT']


def test_val_synthetic_runs_every_leg_its_alt_values_allow():
    legs = validation.validation_legs(_opt(['--val_synthetic', '6']))
    assert [(l.name, l.source) for l in legs] == [('T', ('synthetic', 6))]
    legs = validation.validation_legs(_opt(['--val_synthetic', '6', '--alt_T', '1', '--alt_K', '3', '--alt_F', '2']))
    assert [(l.name, l.K, l.T, l.F) for l in legs] == [('T', 5, 3, 4), ('altT', 5, 1, 4), ('altKF', 3, 3, 2)]
    assert all(l.source == ('synthetic', 6) for l in legs)


def test_validation_clips_are_not_the_training_clips():
    opt = _opt(['--val_synthetic', '2', '--image_size', '16'])
    leg = validation.validation_legs(opt)[0]
    n, batches = validation.leg_batches(leg, opt, 0, 1)
    val = torch.cat(list(batches))
    assert n == 2 and val.shape == (2, 12, 3, 16, 16)
    for rank in range(4):                 # train.py's synthetic clips: --seed + rank
        train = synthetic.make_clips(2, 12, 3, 16, 16, opt.seed + rank)
        assert not np.array_equal(val.numpy(), train)


def test_ragged_batches_keep_clip_order():
    opt = _opt(['--val_synthetic', '5', '--image_size', '8', '--batch_size', '2', '--c_dim', '1'])
    leg = validation.validation_legs(opt)[0]
    n, batches = validation.leg_batches(leg, opt, 0, 1)
    got = list(batches)
    assert [b.shape[0] for b in got] == [2, 2, 1]
    want = synthetic.make_clips(5, 12, 1, 8, 8, opt.seed + validation.VAL_SEED_OFFSET)
    assert np.array_equal(torch.cat(got).numpy(), want)
    # rank 1 of 2 owns clips 3 and 4
    n, batches = validation.leg_batches(leg, opt, 1, 2)
    assert np.array_equal(torch.cat(list(batches)).numpy(), want[3:])


def test_best_snapshot_rule_is_strictly_greater_on_ssim():
    best = (0, 0)
    best, improved = validation.update_best(best, 60.0, 2.5)
    assert improved and best == (60.0, 2.5)
    best, improved = validation.update_best(best, 99.0, 2.5)           # equal SSIM: not better, even with a higher PSNR
    assert not improved and best == (60.0, 2.5)
    best, improved = validation.update_best(best, 10.0, 2.4)
    assert not improved and best == (60.0, 2.5)
    best, improved = validation.update_best(best, 10.0, 2.6)           # higher SSIM wins with a lower PSNR
    assert improved and best == (10.0, 2.6)
    # a resumed run starts from the stored values: a worse first validation does not replace them
    assert validation.update_best((31.0, 4.0), 35.0, 3.9) == ((31.0, 4.0), False)
    # negative sums never beat the initial 0 (the reference's rule)
    assert validation.update_best((0, 0), 5.0, -0.1) == ((0, 0), False)


def test_sum_avg_is_the_sum_over_positions_of_the_mean_over_clips():
    t = np.array([[1., 2., 3.], [3., 4., 5.]])
    assert validation.sum_avg(t) == 2. + 3. + 4.


def test_compute_errors_device_cpu_route_is_compute_errors():
    clips = synthetic.make_clips(2, 6, 3, 20, 24, 17)
    pred, gt = clips[:, :3], clips[:, 3:]
    want = metrics.compute_errors(pred, gt)
    for got in (metrics.compute_errors_device(torch.from_numpy(pred), torch.from_numpy(gt)),
                metrics.compute_errors_device(torch.from_numpy(pred).requires_grad_(), torch.from_numpy(gt)),
                metrics.compute_errors_device(pred, gt)):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def test_psnr_from_sse_is_psnr_uint8():
    rs = np.random.RandomState(0)
    for shape in ((16, 16), (9, 11, 3), (128, 128)):
        a = rs.randint(0, 256, shape).astype(np.uint8)
        b = np.clip(a.astype(int) + rs.randint(-3, 4, shape), 0, 255).astype(np.uint8)
        sse = int(((a.astype(np.int64) - b) ** 2).sum())
        assert metrics.psnr_from_sse(sse, a.size) == metrics.psnr_uint8(a, b)
    assert metrics.psnr_from_sse(0, 10) == float('inf') == metrics.psnr_uint8(a, a)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, n_items, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    parallel.init_from_env(backend='gloo')
    full = np.arange(n_items * 2 * 3, dtype=np.float64).reshape(n_items, 2, 3) / 7.
    mine = full[parallel.shard_slice(n_items, rank, world)]
    got = parallel.gather_rows(mine, n_items)
    np.save(os.path.join(out_dir, 'r%d_n%d.npy' % (rank, n_items)), got)
    import torch.distributed as dist
    dist.destroy_process_group()


@pytest.mark.parametrize('world,n_items', [(2, 5), (3, 7), (3, 2)])
def test_gather_rows_puts_uneven_shards_back_in_order(tmp_path, world, n_items):
    mp.spawn(_gather_worker, args=(world, _free_port(), n_items, str(tmp_path)), nprocs=world, join=True)
    full = np.arange(n_items * 2 * 3, dtype=np.float64).reshape(n_items, 2, 3) / 7.
    for r in range(world):
        got = np.load(tmp_path / ('r%d_n%d.npy' % (r, n_items)))
        assert got.shape == full.shape and np.array_equal(got, full)


def test_gather_rows_single_process_checks_the_shard():
    t = np.ones((4, 3))
    assert np.array_equal(parallel.gather_rows(t, 4), t)
    with pytest.raises(ValueError):
        parallel.gather_rows(t, 5)
