"""Boundary checks of the sharded PPO update that need no GPU: the three entry points are declared in include/go2sim_train.h, parse into the train list
and are exported by the product library; `distributed.allgather_records` returns the ranks' records in rank order on every rank of a world-2 gloo
run and is the identity without a process group."""
import ctypes
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from go2_sim2real_locomotion_rl_amd import capi
from go2_sim2real_locomotion_rl_amd.distributed import allgather_records, broadcast_from_rank0, sum_in_rank_order

SHARD_FUNCS = ("go2sim_ppo_shard_len", "go2sim_ppo_shard_grad", "go2sim_ppo_shard_reduce")


def test_header_declares_the_shard_entry_points():
    assert set(SHARD_FUNCS) <= set(capi.DECLARED_TRAIN_FUNCS)
    assert len(capi.DECLARED_FUNCS) == 53 and not set(SHARD_FUNCS) & set(capi.DECLARED_FUNCS)
    txt = open(capi.TRAIN_HEADER).read()
    # the arguments of the issue, in its order
    grad = txt[txt.index("int go2sim_ppo_shard_grad("):]
    grad = grad[:grad.index(";")]
    pos = [grad.index(a) for a in ("go2sim_ppo_t* h", "const go2sim_ppo_batch_t* batch", "const float* std_dev", "const int32_t* idx_dev", "int n_rows",
                                   "long long n_rows_global", "double* record_dev", "void* stream")]
    assert pos == sorted(pos)
    red = txt[txt.index("int go2sim_ppo_shard_reduce("):]
    red = red[:red.index(";")]
    pos = [red.index(a) for a in ("go2sim_ppo_t* h", "const double* records_dev", "int n_records", "const float* std_dev", "void* stream")]
    assert pos == sorted(pos)
    assert "int go2sim_ppo_shard_len(go2sim_ppo_t* h, size_t* out);" in txt


def test_hip_library_exports_the_shard_entry_points(libs_built):
    lib = ctypes.CDLL(capi.HIP_LIB)
    for name in SHARD_FUNCS:
        assert hasattr(lib, name), f"libgo2sim.so does not export {name}"


def test_ppo_no_longer_lists_multi_gpu_as_out_of_scope():
    txt = open(os.path.join(capi.REPO_ROOT, "go2_sim2real_locomotion_rl_amd", "ppo.py")).read()
    assert "multi-GPU are out of scope" not in txt and "RND and symmetry are out of scope" in txt


def test_allgather_records_is_the_identity_without_a_group():
    rec = torch.arange(7, dtype=torch.float64) / 3
    out = allgather_records(rec)
    assert out.shape == (1, 7) and out.data_ptr() == rec.data_ptr() and torch.equal(out[0], rec)
    assert torch.equal(sum_in_rank_order(rec), rec) and broadcast_from_rank0(rec) is rec


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _record_of(rank, n):
    """float64 values no float32 holds, different on every rank"""
    return (torch.arange(n, dtype=torch.float64) + 1.0) / 7.0 * (1 - 2 * rank) + rank * 1e-9


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = _record_of(rank, n)
        torch.save({"gathered": allgather_records(rec), "group": allgather_records(rec, dist.group.WORLD), "sum": sum_in_rank_order(rec),
                    "bcast": broadcast_from_rank0(rec), "rec_after": rec}, os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_allgather_records_world2_gives_rank_order_on_both_ranks(tmp_path):
    world, n = 2, 1003
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    want = torch.stack([_record_of(r, n) for r in range(world)])
    for r in range(world):
        o = torch.load(tmp_path / f"r{r}.pt")
        assert o["gathered"].dtype == torch.float64 and o["gathered"].shape == (world, n)
        assert torch.equal(o["gathered"], want) and torch.equal(o["group"], want), f"rank {r}"
        assert torch.equal(o["sum"], want[0] + want[1]) and torch.equal(o["bcast"], want[0])
        assert torch.equal(o["rec_after"], want[r]), "the rank's own record is left alone"
