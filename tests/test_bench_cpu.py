"""bench.py's host logic that needs no GPU: the --gpus N self-launch
 and the launch split."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_self_launch_cmd_shape():
    cmd = bench.self_launch_cmd(['--gpus', '8', '--steps', '20', '--warmup', '5'], 8, 29999)
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    i = cmd.index('--nproc-per-node')
    assert cmd[i + 1] == '8'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[cmd.index('--master-port') + 1] == '29999'
    j = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[j + 1:] == ['--gpus', '8', '--steps', '20', '--warmup', '5']


def test_gpus_n_spawns_ranks_and_propagates_failure():
    """`bench.py --gpus 2` outside torchrun starts torchrun as a child with
    two ranks, each of which re-enters bench.py (here each rank fails its own
    argument parsing on purpose, before touching any device), and the
    launcher exits non-zero with the ranks' errors on stderr."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    # torchrun polls its ranks every 0.1 s by default and stops the others as
    # soon as one has failed: a rank that starts a little later than the
    # other is then killed before it reaches its own parser.  Poll after 3 s,
    # by when both have long failed on their own.
    env['PET_MONITOR_INTERVAL'] = '3'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--config', 'nope'],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert 'torch.distributed.run' in r.stderr and '--nproc-per-node 2' in r.stderr
    # both ranks ran bench.py's full argument parser
    assert r.stderr.count("invalid choice: 'nope'") >= 2, r.stderr[-2000:]


def test_rank_count_must_match_gpus():
    """Under a launcher, --gpus must equal the world size the launcher
    started (the driver's `torchrun --nproc-per-node N bench.py --gpus N`)."""
    env = dict(os.environ, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode != 0 and 'launcher started 1 ranks' in r.stderr


def test_dump_outputs_sample_and_files(tmp_path):
    """--dump-outputs: capture_outputs takes a seeded sample of the rows of
    the LAST batch of the slot's last launch (float32, at most DUMP_BYTES),
    with their row numbers and sample ids; write_outputs stores each array
    as <name>.npy (rank-suffixed when there are several ranks)."""
    import numpy as np
    import torch
    batch, nb, b0 = 8, 3, 5
    out = torch.arange(nb * batch * 4 * 4 * 3, dtype=torch.float32).reshape(nb * batch, 4, 4, 3).to(torch.float16)
    order = np.arange(1000, 1000 + (b0 + nb) * batch)
    sl = {'out': out, 'last': (b0, nb, 0)}
    got = bench.capture_outputs(sl, order, batch)
    again = bench.capture_outputs(sl, order, batch)
    assert got['images'].dtype == np.float32 and got['images'].shape == (batch, 4, 4, 3)
    rows = got['rows'].astype(np.int64)
    assert np.array_equal(rows, np.arange(batch))  # the whole batch fits
    assert np.array_equal(got['images'], out[(nb - 1) * batch:].float().numpy())
    assert np.array_equal(got['sample_ids'], order[(b0 + nb - 1) * batch:].astype(np.float64))
    assert all(np.array_equal(got[k], again[k]) for k in got)
    # a batch larger than the budget: a fixed subset of its rows
    big = {'out': torch.zeros((2 * 64, 256, 256, 3), dtype=torch.uint8), 'last': (0, 2, 0)}
    big['out'][64:] = torch.arange(64, dtype=torch.uint8)[:, None, None, None]
    g = bench.capture_outputs(big, np.arange(128), 64)
    keep = bench.DUMP_BYTES // (256 * 256 * 3 * 4)
    assert g['images'].shape == (keep, 256, 256, 3) and g['images'].nbytes <= 64 * 1000 * 1000
    assert np.array_equal(g['images'][:, 0, 0, 0], g['rows']) and np.all(np.diff(g['rows']) > 0)
    assert np.array_equal(g['sample_ids'], 64 + g['rows'])
    bench.write_outputs(str(tmp_path / 'd'), got, 0, 1)
    bench.write_outputs(str(tmp_path / 'd2'), got, 1, 2)
    assert sorted(os.listdir(tmp_path / 'd')) == ['images.npy', 'rows.npy', 'sample_ids.npy']
    assert np.array_equal(np.load(tmp_path / 'd' / 'images.npy'), got['images'])
    assert sorted(os.listdir(tmp_path / 'd2')) == ['images.rank1.npy', 'rows.rank1.npy', 'sample_ids.rank1.npy']
