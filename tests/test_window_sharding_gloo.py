"""Band sharding on CPU: two gloo ranks, each renders ALL sample indices of ITS band of rows with the oracle renderer; the product's
stepping and reduction code (vspg-pbrt-v4_amd/sharding.py: window_bands, BandShard, ShardSync, frame_end_allreduce) runs
unchanged.  A pixel gets every one of its samples from one rank and 0 from the other, so the all-reduced film and the VSP buffer
are ONE renderer's bit for bit -- image-space buffer updates (wave counters 1, 2, 4) fall inside the run."""
import importlib.util
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

W, H, STEPS = 48, 40, 5


def _load_sharding():
    spec = importlib.util.spec_from_file_location("vspg_sharding", os.path.join(ROOT, "vspg-pbrt-v4_amd", "sharding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("yres", [1, 7, 8, 76, 1080, 2160])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_window_bands_cover_every_row_once(yres, world):
    bands = _load_sharding().window_bands(yres, world)
    assert len(bands) == world
    rows = np.zeros(yres, dtype=int)
    for y0, y1 in bands:
        assert 0 <= y0 <= y1 <= yres
        rows[y0:y1] += 1
    assert np.all(rows == 1)
    assert bands[0][0] == 0 and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))       # in order, no gaps
    assert all(y % 8 == 0 or y == yres for _, y in bands)                                   # boundaries on the tile grid


def _worker(rank, world, port, out_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    from oracle_band_shard import OracleBandShard
    from oracle_shard import host_tensor
    sh = _load_sharding()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    scene = oracle_lib.fog_box_scene(W, H)
    prm = oracle_lib.app_f_params()
    o = oracle_lib.OracleRenderer(scene, prm, W, H, seed=3)          # shard_count = 1: every sample index of the band
    r = OracleBandShard(o)
    sync = sh.ShardSync(dist, r, world, torch, device=None, wrap=host_tensor(torch), waves_per_step=1)
    band = sh.BandShard(r, W, H, rank, world)
    assert (band.y0, band.y1) == sh.window_bands(H, world)[rank]
    for step in range(STEPS):
        band.render(step, step + 1)
        sync.post_process_step()
    film = torch.from_numpy(o.film_f64().copy())
    paths = o.counters()["paths"]
    sh.frame_end_allreduce(dist, film, world)
    total_paths, = sh.sum_over_ranks(dist, [paths], world, "cpu")
    vsp, ready = o.vsp_buffer()
    np.save(out_path % rank, vsp)
    if rank == 0:
        np.save(out_path % 9, film.numpy())
        assert total_paths == W * H * STEPS and ready
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_band_sharded_render_equals_one_renderer(tmp_path):
    import oracle_lib
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "out%d.npy")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    one = oracle_lib.OracleRenderer(oracle_lib.fog_box_scene(W, H), oracle_lib.app_f_params(), W, H, seed=3)
    for step in range(STEPS):
        one.render_wave(step, step + 1, 1)
        one.post_process_wave()
    film = np.load(out % 9)
    assert np.array_equal(film.view(np.uint64), one.film_f64().view(np.uint64))
    vsp = one.vsp_buffer()[0]
    assert len(np.unique(vsp)) > 10                                   # the buffer really was updated from the statistics
    for rank in range(world):
        assert np.array_equal(np.load(out % rank).view(np.uint32), vsp.view(np.uint32))
    one.close()


def test_band_mode_refuses_in_loop_training():
    sh = _load_sharding()

    class Training:
        def training_stats(self):
            return {"training": 1}

        def render_window(self, *a):
            raise AssertionError("rendered")
    with pytest.raises(RuntimeError, match="band sharding does not cover in-loop training"):
        sh.BandShard(Training(), W, H, 0, 2)
    with pytest.raises(TypeError):                    # a wrapper that cannot answer the question is refused, not waved through
        sh.BandShard(object(), W, H, 0, 2)
