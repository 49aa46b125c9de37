"""One rank of a band-sharded render on the HIP renderer, rehearsed on ONE card (both ranks on device 0, collectives over gloo --
the shape of bench.py's VSPG_BENCH_REHEARSE): every rank renders all sample indices of its band of rows (sharding.BandShard),
the statistics exchange (ShardSync) and the frame-end film all-reduce run as they do under sample-index sharding, rank 0 saves the
summed film and its VSP buffer.  Started by tests/test_window_gpu.py through torch.distributed.run; test infrastructure only."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402


class DevArray:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}


def main():
    W, H, steps, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo")
    pkg = load_package()
    pkg.load()
    spec = importlib.util.spec_from_file_location("vspg_sharding", os.path.join(ROOT, "vspg-pbrt-v4_amd", "sharding.py"))
    sh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sh)
    dev = torch.device("cuda", 0)
    r = pkg.Renderer(pkg.fog_box_scene(W, H), pkg.app_f_params(), W, H, seed=3, device=0)      # shard_count = 1
    fptr, fn = r.film_ptr()
    film = torch.as_tensor(DevArray(fptr, fn), device=dev)
    sync = sh.ShardSync(dist, r, world, torch, device=dev, waves_per_step=1)
    stream = torch.cuda.current_stream().cuda_stream
    band = sh.BandShard(r, W, H, rank, world)
    for step in range(steps):
        band.render(step, step + 1, stream)
        sync.post_process_step(stream)
    sh.frame_end_allreduce(dist, film, world, r, stream, torch=torch, device=dev)
    torch.cuda.synchronize()
    paths, = sh.sum_over_ranks(dist, [r.counters()["paths"]], world, "cpu")
    if rank == 0:
        np.savez(out, film=film.view(H, W, 4).cpu().numpy(), vsp=r.vsp_buffer(stream)[0], paths=np.array([paths]))
    dist.barrier()
    r.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
