"""Multi-GPU sharding helpers.

Besides the advantage statistics, the reference's env has ONE curriculum level and ONE set of "global" DR scalars for all its envs
(go2_env_walk.py:458-463, 737-756, 803-848).  `sync_env_globals` keeps that true for a batch sharded over ranks: an all-reduce of the four
curriculum counters (+ the friction-throttle counter), the same state machine on every rank, and a broadcast of rank 0's draws.

Environments are fully independent, so the hot path shards as contiguous blocks of envs per GPU with NO
physics traffic.  The only collective the path needs is the rollout advantage-normalisation statistics:
an all-gather of [sum, sum of squared deviations from the rank's mean, count] (3 floats per rank) over RCCL/xGMI (backend "nccl" on ROCm,
"gloo" in the CPU tests).  The reference has no distributed code on this path (its only multi-GPU artefact
is examples/ddp_multi_gpu.py:36-90, one independent scene per rank with seed=local_rank)."""
import torch
import torch.distributed as dist


def shard_seed(seed: int, rank: int) -> int:
    """Per-rank RNG stream (examples/ddp_multi_gpu.py:58 uses seed=local_rank)."""
    return int(seed) + int(rank)


def shard_envs(total_envs: int, world_size: int, rank: int):
    """Contiguous block of envs owned by `rank` -> (start, count)."""
    base, rem = divmod(total_envs, world_size)
    count = base + (1 if rank < rem else 0)
    start = rank * base + min(rank, rem)
    return start, count


def merge_moments(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[sum, M2, count] of the union of two sets from theirs, M2 the sum of squared deviations from the set's own mean (Chan et al.):
    M2 = M2_a + M2_b + (mean_b - mean_a)^2 n_a n_b / (n_a + n_b).  Unlike a sum of squares, nothing here is of the size of mean^2."""
    n = a[2] + b[2]
    delta = b[0] / b[2] - a[0] / a[2]
    return torch.stack([a[0] + b[0], a[1] + b[1] + delta * delta * (a[2] * b[2] / n), n])


def is_multi(group=None) -> bool:
    """True inside a process group of more than one rank."""
    return dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1


def allgather_records(record: torch.Tensor, group=None) -> torch.Tensor:
    """Every rank's `record` (a flat tensor of the same length on every rank) as [world][len] in rank order: ONE all-gather.  Under "nccl" the device
    tensor goes through ``all_gather_into_tensor`` on torch's current stream (RCCL over xGMI; nothing is copied to the host); under "gloo" (CPU tests,
    one-GPU rehearsal) a device tensor is staged through the host, as sync_env_globals does.  With a single process it is the record itself, [1][len]."""
    record = record.reshape(-1)
    if not is_multi(group):
        return record.view(1, -1)
    world = dist.get_world_size(group)
    staged = record.is_cuda and dist.get_backend(group) != "nccl"
    src = (record.cpu() if staged else record).contiguous()
    out = torch.empty(world * src.numel(), device=src.device, dtype=src.dtype)
    dist.all_gather_into_tensor(out, src, group=group)
    out = out.view(world, src.numel())
    return out.to(record.device) if staged else out


def sum_in_rank_order(x: torch.Tensor, group=None) -> torch.Tensor:
    """The ranks' `x` added in rank order (one all-gather): every rank gets the same bits.  Identity for a single process."""
    parts = allgather_records(x, group)
    s = parts[0].clone()
    for r in range(1, parts.shape[0]):
        s += parts[r]
    return s.view(x.shape)


def broadcast_from_rank0(x: torch.Tensor, group=None) -> torch.Tensor:
    """Rank 0's `x` on every rank (a new tensor on x's device); staged through the host under "gloo".  Identity for a single process."""
    if not is_multi(group):
        return x
    src = dist.get_global_rank(group, 0) if group is not None else 0
    staged = x.is_cuda and dist.get_backend(group) != "nccl"
    buf = (x.cpu() if staged else x.clone()).contiguous()
    dist.broadcast(buf, src=src, group=group)
    return buf.to(x.device) if staged else buf


def _merge_ranks(m: torch.Tensor, group=None) -> torch.Tensor:
    """One all-gather of 3 values per rank, merged in rank order so that every rank gets the same bits; identity for a single process."""
    if is_multi(group):
        world = dist.get_world_size(group)
        out = allgather_records(m, group)
        g = out[0].clone()
        for r in range(1, world):
            g = merge_moments(g, out[r])
        return g
    return m


def global_mean_std(x: torch.Tensor, group=None):
    """Mean / unbiased std (``torch.std``) of `x` over all ranks, via ONE all-gather of 3 values per rank.  The moments are the library's
    (go2sim_rollout_compute_returns): float64, the squared deviations taken in a second pass, so that both advantage normalisations of the
    package agree."""
    xd = x.reshape(-1).to(torch.float64)
    s = xd.sum()
    d = xd - s / xd.numel()
    m = _merge_ranks(torch.stack([s, (d * d).sum(), torch.tensor(float(xd.numel()), device=x.device, dtype=torch.float64)]), group)
    n = m[2]
    var = torch.clamp(m[1] / torch.clamp(n - 1.0, min=1.0), min=0.0)
    return (m[0] / n).to(torch.float32), torch.sqrt(var).to(torch.float32)


def normalize_advantages(adv: torch.Tensor, group=None, eps: float = 1e-8) -> torch.Tensor:
    """rsl_rl 2.2.4 PPO: ``(adv - adv.mean()) / (adv.std() + 1e-8)`` with the statistics taken over all ranks -- the formula of
    ``go2sim_rollout_normalize`` (unbiased std, eps added to the std)."""
    mean, std = global_mean_std(adv, group)
    return (adv - mean) / (std + eps)


def allgather_moments(moments3: torch.Tensor, group=None) -> torch.Tensor:
    """Global [sum, sum of squared deviations from the mean, count] from the per-rank moments of go2sim_rollout_compute_returns (float64[3]):
    one all-gather of 3 values per rank (RCCL over xGMI with backend "nccl", gloo in the CPU tests), merged in rank order (merge_moments) so that
    every rank gets the same bits."""
    return _merge_ranks(moments3, group)


def sync_env_globals(sim, group=None, stream=None, initial=False):
    """One batch sharded over ranks, one curriculum / one set of global DR scalars.  `sim` is a capi.Go2Sim configured with
    ``shared_globals=True`` (GO2SIM_IC_SHARED_GLOBALS).  Call it on every rank at the same cadence (once per rollout):
      1. this shard's increments of [episodes, time-outs, tracking sum, tracking n, throttle resets] (go2_env_walk.py:460-463, 712-715, 744)
      2. all-reduce(sum) of those 5 float64 (RCCL over xGMI with backend "nccl"; gloo in the CPU tests)
      3. every rank runs _maybe_update_curriculum_on_reset / sample_level / the global DR draws on the SAME summed counters
      4. broadcast of rank 0's draws (friction, mass shift, COM shift, leg-mass shifts and the sampled DR level t_sample: 10 float64), applied
         to all envs of every shard.
    Returns (summed counters, the 10 scalars now in force; device tensors under nccl).  Without a process group it degenerates to the single-shard case.
    Call it ONCE with ``initial=True`` between env_configure and the constructor's env_reset as well (Go2Env and bench.make_sim do): that first apply draws
    t_sample at level_init and the global scalars on rank 0 -- with the batch's env count as the friction-throttle increment, as the constructor's reset_idx
    counts it -- and every shard starts where the single-process env starts."""
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    src = (dist.get_global_rank(group, 0) if group is not None else 0) if multi else 0
    if multi and dist.get_backend(group) == "nccl":
        # RCCL: counters and scalars stay on the device from the shard's Glob to the collective and back (three single-thread kernels of the library
        # around two collectives, all ordered on torch's current stream); nothing is copied to the host and nothing synchronises
        dev = torch.device("cuda", torch.cuda.current_device())
        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        counters = torch.empty(5, dtype=torch.float64, device=dev)
        dr = torch.empty(10, dtype=torch.float64, device=dev)
        sim.env_sync_counters_dev(counters, stream)
        if initial:
            counters[4] += float(sim.n_envs)
        dist.all_reduce(counters, op=dist.ReduceOp.SUM, group=group)
        sim.env_sync_apply_dev(counters, dr, stream)
        dist.broadcast(dr, src=src, group=group)
        sim.env_set_global_dr_dev(dr, stream)
        return counters, dr
    counters = torch.from_numpy(sim.env_sync_counters(stream))       # gloo (CPU tests, rehearsal) and the single-shard case: host arrays
    if initial:
        counters[4] += float(sim.n_envs)
    if multi:
        dist.all_reduce(counters, op=dist.ReduceOp.SUM, group=group)
    summed = counters.numpy()
    dr = torch.from_numpy(sim.env_sync_apply(summed, stream))
    if multi:
        dist.broadcast(dr, src=src, group=group)
    dr = dr.numpy()
    sim.env_set_global_dr(dr, stream)
    return summed, dr
