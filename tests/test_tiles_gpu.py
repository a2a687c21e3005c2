"""The HIP library's rough-terrain kernels (include/go2sim_tiles.h) against the float32 restatement tests/tiles_ref.py, bit for bit.

go2sim_tiles_query on the 6 x 5 and 9 x 4 fields of tests/tiles_cases.py (a non-square field shows an axis swap): cell corners, edge midpoints, interior
points, points outside on all four sides (they clamp), l exactly n - 2, and +-inf / NaN coordinates (cell 0 or n - 2 with f = 0: a finite height, nothing
faults); the int16 and the float32 form of the field give the same bits.  k_env_tile_spawn through go2sim_env_reset / go2sim_env_reset_idx: 5 and 70 envs
(a partial wavefront, more than one), reset masks all / none / sparse, grids 1 x 1, 2 x 2, 3 x 1 and a tile whose jitter is <= 0 along x only; envs that are
not reset keep their record, the reset base stands on the spawn point, equal calls give equal bits."""
import numpy as np
import pytest
import torch

import tiles_cases as TC
import tiles_ref as R
from go2_sim2real_locomotion_rl_amd.capi import C, Go2Sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def query(sim, pts):
    xy = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(DEV)
    out = torch.full((len(pts),), float("nan"), device=DEV)
    sim.tiles_query(xy, out, len(pts))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def env_buf(sim, name, k, dtype=torch.float32):
    t = torch.zeros(sim.n_envs, k, dtype=dtype, device=DEV)
    sim.env_get(C["GO2SIM_EB_" + name], t)
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("name", sorted(TC.FIELDS))
def test_query_is_the_restatement_bit_for_bit(hip_lib, blob, name):
    rows, cols, hs, vs, org = TC.FIELDS[name]
    hf = TC.field(name)
    pts, n_finite = TC.query_points(name)
    want = R.ground_height(R.metres(hf, vs), org, hs, pts[:, 0], pts[:, 1])
    assert np.isfinite(want).all(), "the stated rule: a finite field gives a finite height at any coordinate"
    sim = Go2Sim(hip_lib, blob, 1, 0, 1)
    sim.set_terrain(hf, hs, vs, org)
    got = query(sim, pts)
    bad = np.flatnonzero(bits(got) != bits(want))
    print(f"{name}: {len(pts)} points ({len(pts) - n_finite} non-finite), {len(bad)} differ")
    assert not len(bad), (pts[bad], got[bad], want[bad])
    # corners read the cell itself, so the axes are not swapped; the last row and column clamp to l = n - 2 and read their neighbour, as in the reference
    corner = R.metres(hf, vs)
    corner[-1, :] = corner[-2, :]
    corner[:, -1] = corner[:, -2]
    assert np.array_equal(bits(got[:rows * cols]), bits(corner.reshape(-1)))
    # the float32 form of the same field: the same bits
    sim2 = Go2Sim(hip_lib, blob, 1, 0, 1)
    sim2.set_terrain_f32(R.metres(hf, vs), hs, org)
    assert np.array_equal(bits(query(sim2, pts)), bits(want))
    # equal calls, equal bits; n = 0 launches nothing
    assert np.array_equal(bits(query(sim, pts)), bits(got))
    sim.tiles_query(None, None, 0)


def test_query_and_float_field_refusals(hip_lib, blob):
    from go2_sim2real_locomotion_rl_amd.capi import Go2SimError

    sim = Go2Sim(hip_lib, blob, 1, 0, 1)
    xy, out = torch.zeros(1, 2, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(Go2SimError):
        sim.tiles_query(xy, out, 1)                                        # no heightfield on the handle
    hf = np.zeros((4, 4), np.float32)
    for bad in (np.nan, np.inf):
        h = hf.copy(); h[1, 2] = bad
        with pytest.raises(Go2SimError):
            sim.set_terrain_f32(h, 0.25, (0.0, 0.0, 0.0))
    with pytest.raises(Go2SimError):
        sim.set_terrain_f32(hf[:1], 0.25, (0.0, 0.0, 0.0))                # fewer than 2 rows
    f, i, _ = TC.tile_env_cfg(1, TC.grid_terrain_cfg("1x1")[1])
    sim.env_configure(f, i)
    with pytest.raises(Go2SimError):
        sim.env_reset()                                                    # tile mode without a heightfield
    i[C["GO2SIM_IC_USE_TERRAIN"]] = 1
    with pytest.raises(Go2SimError):
        sim.env_configure(f, i)                                            # the stair env's terrain terms and the tile mode exclude each other


def make_tile_sim(hip_lib, blob, n, grid_name, seed):
    hf, grid = TC.grid_terrain_cfg(grid_name)
    sim = Go2Sim(hip_lib, blob, n, 0, seed)
    sim.set_terrain(hf, TC.GRID_HS, TC.GRID_VS, grid["origin"])
    f, i, _ = TC.tile_env_cfg(n, grid)
    sim.env_configure(f, i)
    g = dict(grid, base_z=0.45, spawn_offset=0.05)
    return sim, R.metres(hf, TC.GRID_VS), g


def records(sim):
    return env_buf(sim, "SPAWN_POS", 3), env_buf(sim, "TILE_ROW", 1, torch.int32)[:, 0], env_buf(sim, "TILE_COL", 1, torch.int32)[:, 0]


@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("grid_name", sorted(TC.GRIDS))
def test_spawn_is_the_restatement_bit_for_bit(hip_lib, blob, grid_name, n):
    seed = 0x1234567890 + n
    sim, H, g = make_tile_sim(hip_lib, blob, n, grid_name, seed)
    pos0, row0, col0 = records(sim)
    assert not pos0.any() and not row0.any() and not col0.any()

    def want(call):
        return R.spawn(H, g["origin"], TC.GRID_HS, g, R.spawn_words(n, seed, call))

    # mask "all": the constructor's reset
    sim.env_reset()
    assert sim.env_globals().reset_calls == 1
    pos, row, col = records(sim)
    wpos, wrow, wcol = want(0)
    assert np.array_equal(bits(pos), bits(wpos)) and np.array_equal(row, wrow) and np.array_equal(col, wcol)
    assert np.array_equal(bits(env_buf(sim, "BASE_POS", 3)), bits(wpos)), "the reset base stands on the spawn point"
    assert row.max() < g["n_rows"] and col.max() < g["n_cols"]
    if n == 70 and g["n_rows"] > 1:
        assert len(set(row)) == g["n_rows"]                               # every tile row is drawn
    centre_x = np.float32(g["origin"][0]) + (row.astype(np.float32) + np.float32(0.5)) * np.float32(g["size"][0])
    if g["jitter"][0] <= 0:
        assert np.array_equal(bits(pos[:, 0]), bits(centre_x)), "no jitter room along x: the tile centre"
        assert (pos[:, 1] != np.float32(g["origin"][1]) + (col.astype(np.float32) + np.float32(0.5)) * np.float32(g["size"][1])).any()
    else:
        assert (np.abs(pos[:, 0] - centre_x) <= g["jitter"][0] + 2.0 * R.ulp32(g["origin"][0])).all() and (pos[:, 0] != centre_x).any()   # (the sum rounds once)
    # mask "none": nothing moves, no reset call is counted
    sim.env_reset_idx(torch.zeros(0, dtype=torch.int32, device=DEV), 0)
    assert sim.env_globals().reset_calls == 1
    assert all(np.array_equal(a, b) for a, b in zip(records(sim), (pos, row, col)))
    # mask "sparse": the listed envs draw with the next reset call's key, the others keep their record
    idx = np.arange(n)[::3][: max(1, n // 4)]
    sim.env_reset_idx(torch.from_numpy(idx.astype(np.int32)).to(DEV), len(idx))
    assert sim.env_globals().reset_calls == 2
    pos2, row2, col2 = records(sim)
    wpos2, wrow2, wcol2 = want(1)
    keep = np.setdiff1d(np.arange(n), idx)
    assert np.array_equal(bits(pos2[idx]), bits(wpos2[idx])) and np.array_equal(row2[idx], wrow2[idx]) and np.array_equal(col2[idx], wcol2[idx])
    assert np.array_equal(bits(pos2[keep]), bits(pos[keep])) and np.array_equal(row2[keep], row[keep]) and np.array_equal(col2[keep], col[keep])
    # equal calls give equal bits
    twin, _, _ = make_tile_sim(hip_lib, blob, n, grid_name, seed)
    twin.env_reset()
    twin.env_reset_idx(torch.from_numpy(idx.astype(np.int32)).to(DEV), len(idx))
    assert all(np.array_equal(a, b) for a, b in zip(records(twin), (pos2, row2, col2)))
