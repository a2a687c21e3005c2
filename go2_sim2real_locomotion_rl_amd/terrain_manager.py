"""TerrainManager -- the reference's examples/locomotion/terrain_manager.py on the device.

Same constructor, public methods and attributes (``enabled``, ``build_terrain_morph``, ``post_build``, ``sample_spawn``, ``check_boundary``,
``get_height_at_robot``, ``get_env_tile_rows``, ``get_terrain_type_string``, ``max_wander``), so the reference's env file
(go2_env_Omni_kplearn_varied_terrain.py) runs on the ``genesis`` alias with this class, and ``Go2Env.terrain`` is one.  Two ways of use:

  * stand-alone (the reference's env file on the shim): every method is torch arithmetic on ``device`` in the float32 operation order of
    include/go2sim_tiles.h -- the reference's ``_query_height_batch`` copies the positions to the host and interpolates with numpy on every env
    step, ``_sample_spawn_grid`` loops over the reset envs in Python; nothing here synchronises with the host;
  * bound to a ``Go2Env`` (``bind``): the library draws the spawn inside its reset and evaluates the ground height and the boundary inside the
    step, and the manager's per-env records are read-outs of the library's (GO2SIM_EB_SPAWN_POS / _TILE_ROW / _TILE_COL), ``get_height_at_robot``
    is go2sim_tiles_query.

``terrain_tiles.tile_layout(cfg)`` holds the arithmetic both share with configs.flatten_walk_cfg: grid shape, tile size, origin, max_wander and jitter as the
reference forms them (python floats)."""
import numpy as np
import torch

from .capi import Go2SimError
from .terrain_tiles import install_terrain, is_tile_terrain_cfg, tile_layout  # noqa: F401  (re-exported)


def bilinear_height(hf_m, origin_xy, hs, wx, wy):
    """Ground height of include/go2sim_tiles.h in torch float32, same operations in the same order: hf_m [rows][cols] metres on the points'
    device, wx / wy float32 [n]."""
    rows, cols = hf_m.shape
    ox, oy, hs = (torch.tensor(v, dtype=torch.float32, device=wx.device) for v in (origin_xy[0], origin_xy[1], hs))

    def axis(w, o, n):
        q = (w - o) / hs
        top = float(n - 2)
        l = torch.where(q > 0, q, torch.zeros_like(q))
        l = torch.where(q >= top, torch.full_like(q, top), l)
        i = l.to(torch.int64)
        return i, l - i.to(torch.float32)

    ix, fx = axis(wx.to(torch.float32), ox, rows)
    iy, fy = axis(wy.to(torch.float32), oy, cols)
    gx, gy = 1.0 - fx, 1.0 - fy
    h = (hf_m[ix, iy] * gx) * gy
    h = h + (hf_m[ix + 1, iy] * fx) * gy
    h = h + (hf_m[ix, iy + 1] * gx) * fy
    h = h + (hf_m[ix + 1, iy + 1] * fx) * fy
    return h


class TerrainManager:
    def __init__(self, terrain_cfg, num_envs, device=None):
        self.cfg = terrain_cfg or {}
        self.enabled = bool(self.cfg.get("enabled", False))
        if device is None:
            from . import genesis_shim as gs

            device = gs.device if gs.device is not None else "cpu"
        self.device = torch.device(device)
        self.num_envs = num_envs
        self._env = None
        if not self.enabled:
            return
        L = self._layout = tile_layout(self.cfg)
        self.use_custom_heightmap = L["mode"] == "heightmap"
        self.horizontal_scale, self.vertical_scale = L["horizontal_scale"], L["vertical_scale"]
        self.spawn_height_offset, self.boundary_margin = L["spawn_height_offset"], L["boundary_margin"]
        self.subterrain_types, self.n_rows, self.n_cols = L["subterrain_types"], L["n_rows"], L["n_cols"]
        self.subterrain_size, self.max_wander = L["subterrain_size"], L["max_wander"]
        self.randomize = bool(L.get("randomize", False))
        self._terrain_size_x, self._terrain_size_y = L["n_rows"] * L["subterrain_size"][0], L["n_cols"] * L["subterrain_size"][1]
        self._flat_row_indices = [r for r, row in enumerate(self.subterrain_types or []) if all(t == "flat_terrain" for t in row)]
        self._height_field_np = L["height_field"]
        self._terrain_origin = np.array(L["origin"])
        self._tile_row = torch.zeros(num_envs, device=self.device, dtype=torch.long)
        self._tile_col = torch.zeros(num_envs, device=self.device, dtype=torch.long)
        self._spawn_pos = torch.zeros(num_envs, 3, device=self.device, dtype=torch.float32)
        self._height_field = self._height_field_np            # raw units, numpy (the reference's attribute); grid mode: after post_build
        self._hf_m = None                                     # metres, float32, on the device
        self._tile_centers = None
        if not self.use_custom_heightmap:
            r, c = torch.arange(self.n_rows, dtype=torch.float64), torch.arange(self.n_cols, dtype=torch.float64)
            centers = torch.zeros(self.n_rows, self.n_cols, 3, dtype=torch.float64)
            centers[:, :, 0] = (self._terrain_origin[0] + (r + 0.5) * self.subterrain_size[0])[:, None]
            centers[:, :, 1] = (self._terrain_origin[1] + (c + 0.5) * self.subterrain_size[1])[None, :]
            self._tile_centers = centers.to(device=self.device, dtype=torch.float32)
        else:
            self._cache_field(self._height_field_np)

    # ---- build ------------------------------------------------------------------------------------------------------------------------
    def build_terrain_morph(self):
        """The gs.morphs.Terrain morph; call before scene.build()."""
        if not self.enabled:
            return None
        from . import genesis_shim as gs

        kw = dict(pos=tuple(self._terrain_origin), horizontal_scale=self.horizontal_scale, vertical_scale=self.vertical_scale,
                  name=self.cfg.get("terrain_name", None))
        if self.use_custom_heightmap:
            return gs.morphs.Terrain(height_field=self._height_field_np, **kw)
        kw.update(n_subterrains=(self.n_rows, self.n_cols), subterrain_size=self.subterrain_size, subterrain_types=self.subterrain_types,
                  randomize=self.randomize)
        if self.cfg.get("subterrain_parameters", None) is not None:
            kw["subterrain_parameters"] = self.cfg["subterrain_parameters"]
        return gs.morphs.Terrain(**kw)

    def _cache_field(self, hf_raw):
        self._height_field = np.array(hf_raw, dtype=np.float32)
        metres = self._height_field * np.float32(self.vertical_scale)               # f32(hf) * f32(vertical_scale), as the library forms its copy
        self._hf_m = torch.from_numpy(np.ascontiguousarray(metres)).to(self.device)

    def post_build(self, terrain_entity):
        """Call after scene.build(): takes the generated field from the terrain entity (grid mode)."""
        if not self.enabled or (self.use_custom_heightmap and self._hf_m is not None):
            return
        holders = [h for h in (terrain_entity, getattr(terrain_entity, "morph", None)) if h is not None]
        found = [getattr(h, a) for h in holders for a in ("height_field", "heightfield", "_height_field", "hf") if getattr(h, a, None) is not None]
        hf = found[0] if found else None
        if hf is None:
            raise Go2SimError("the terrain entity exposes no height field: ground heights would read 0")
        self._cache_field(hf)

    def bind(self, env):
        """Go2Env: the per-env records and the height query are the library's from here on."""
        self._env = env

    # ---- per-env records --------------------------------------------------------------------------------------------------------------
    @property
    def _env_spawn_pos(self):
        return self._spawn_pos if self._env is None else self._env._env_view("SPAWN_POS", 3)

    @property
    def _env_tile_row(self):
        return self._tile_row if self._env is None else self._env._env_view("TILE_ROW", 1, torch.int32).long()

    @property
    def _env_tile_col(self):
        return self._tile_col if self._env is None else self._env._env_view("TILE_COL", 1, torch.int32).long()

    # ---- spawn and boundary -----------------------------------------------------------------------------------------------------------
    def sample_spawn(self, envs_idx, base_init_z=0.42):
        """A spawn position [n, 3] for each env of `envs_idx`: a uniform tile and a uniform jitter inside it (the whole field in heightmap mode),
        z = ground + base_init_z + spawn_height_offset.  Draws with torch's generator in the reference's order: rows, columns, x jitter, y jitter."""
        if not self.enabled:
            return None
        if self._env is not None:
            raise Go2SimError("this manager belongs to a Go2Env: the library draws the spawn inside reset / reset_idx (include/go2sim_tiles.h)")
        n = len(envs_idx)
        if n == 0:
            return None
        idx = torch.as_tensor(envs_idx, device=self.device).long()
        pos = torch.zeros(n, 3, device=self.device, dtype=torch.float32)
        if self.use_custom_heightmap:
            rows = cols = torch.zeros(n, device=self.device, dtype=torch.long)
        else:
            rows = torch.randint(0, self.n_rows, (n,), device=self.device)
            cols = torch.randint(0, self.n_cols, (n,), device=self.device)
            pos[:] = self._tile_centers[rows, cols]
        jx, jy = self._layout["jitter"]
        if jx > 0:
            pos[:, 0] += (torch.rand(n, device=self.device) * 2 - 1) * jx
        if jy > 0:
            pos[:, 1] += (torch.rand(n, device=self.device) * 2 - 1) * jy
        pos[:, 2] = self._query_height_batch(pos[:, 0], pos[:, 1]) + base_init_z + self.spawn_height_offset
        self._spawn_pos[idx] = pos
        self._tile_row[idx], self._tile_col[idx] = rows, cols
        return pos

    def check_boundary(self, base_pos_xy):
        """bool [num_envs]: the base is further than max_wander from its spawn point (strictly)."""
        if not self.enabled:
            return torch.zeros(self.num_envs, device=self.device, dtype=torch.bool)
        d = base_pos_xy.to(torch.float32) - self._env_spawn_pos[:, :2]
        return torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) > self.max_wander

    # ---- height queries ---------------------------------------------------------------------------------------------------------------
    def _query_height_batch(self, world_x, world_y):
        n = len(world_x)
        if self._env is not None:
            xy = torch.stack([world_x, world_y], dim=1).to(device=self.device, dtype=torch.float32).contiguous()
            out = torch.empty(n, device=self.device, dtype=torch.float32)
            self._env._sim.tiles_query(xy, out, n, torch.cuda.current_stream(self.device).cuda_stream)
            return out
        if self._hf_m is None:
            return torch.zeros(n, device=self.device, dtype=torch.float32)
        return bilinear_height(self._hf_m, self._terrain_origin, self.horizontal_scale, world_x.to(self.device), world_y.to(self.device))

    def get_height_at_robot(self, base_pos_xy):
        """(num_envs, 2) -> (num_envs,)"""
        return self._query_height_batch(base_pos_xy[:, 0], base_pos_xy[:, 1])

    # ---- info -------------------------------------------------------------------------------------------------------------------------
    def get_env_tile_rows(self):
        return self._env_tile_row

    def get_terrain_type_string(self, env_idx):
        if self.use_custom_heightmap:
            return "custom_heightmap"
        return self.subterrain_types[int(self._env_tile_row[env_idx].item())][int(self._env_tile_col[env_idx].item())]
