"""world_size-2 test of `radiometry.reduce_counts` on the gloo backend (no device), in the manner of tests/test_dist_gloo.py:
under --multiple_gpus every rank holds the histogram of its own shard, and the `auto` band ranges must come out alike on all of
them - the percentiles of the summed counts, which are those of the whole dataset."""
import os
import socket
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    from diffusionremotesensing_amd import dist
    dist.init_process_group("gloo")
    try:
        _case(rank, world, out_dir)
    finally:
        dist.destroy_process_group()


def _dataset():
    """(4, 2, 8, 8) uint16: band 0 dark (a few hundred values), band 1 spread over the whole range."""
    rng = np.random.default_rng(11)
    dark = np.minimum(rng.gamma(2.0, 150.0, (4, 1, 8, 8)), 65535).astype(np.uint16)
    wide = rng.integers(0, 65536, (4, 1, 8, 8)).astype(np.uint16)
    return np.concatenate([dark, wide], axis=1)


def _case(rank, world, out_dir):
    import radiometry_oracle as RO
    from diffusionremotesensing_amd import radiometry as R
    data = _dataset()
    mine = torch.from_numpy(RO.histogram(data[rank::world]))  # what drs_hist_u16 gives this rank's shard
    whole = RO.histogram(data)
    assert not np.array_equal(mine.numpy(), whole)
    got = R.reduce_counts(mine)
    assert got is mine and got.dtype == torch.int64 and np.array_equal(got.numpy(), whole)
    table = R.range_from_counts(got, 2.0, 98.0)
    assert table.tolist() == RO.range_from_counts(whole, 2.0, 98.0).tolist()
    np.save(os.path.join(out_dir, f"table{rank}.npy"), table)


def test_reduce_counts_world_2(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(tmp_path / f"table{r}.npy") for r in (0, 1))
    assert a.shape == (2, 2) and np.array_equal(a, b)  # every rank normalises alike
