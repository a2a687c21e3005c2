"""go2_sim2real_locomotion_rl_amd -- MI355X-native vectorised Go2 locomotion environment.

Drop-in for the hot path of saifahmadgit/go2-sim2real-locomotion-rl:
``Go2Env.step()/reset()`` over ``gs.Scene.step()``."""
from .capi import C, Go2Sim, Go2SimError, load_hip_lib  # noqa: F401
from .configs import (flatten_base_cfg, flatten_walk_cfg, get_crouch_cfgs, get_jump_cfgs, get_stair_cfgs,  # noqa: F401
                      get_rough_cfgs, get_stair_info_cfg, get_stair_info_cfgs, get_stair_lidar_cfgs, get_stairwell_cfgs, get_walk_cfgs)
from .contact_terms import ContactTerms  # noqa: F401
from .distillation import (Distillation, StudentTeacher, StudentTeacherRecurrent, distill_windows, rdistill_schedule,  # noqa: F401
                           teacher_state_from_checkpoint)
from .distributed import allgather_records, shard_envs, shard_seed  # noqa: F401
from .evaluation import EvalStats, Evaluator, bin_metrics, command_grid  # noqa: F401
from .eval_io import load_cfgs, read_checkpoint, save_cfgs, save_checkpoint  # noqa: F401
from .go2_env import Go2Env, init  # noqa: F401
from .lidar import LidarScan  # noqa: F401
from .model_blob import load_model_json, pack_model  # noqa: F401
from .normalization import EmpiricalNormalization  # noqa: F401
from .policy import ActorCritic, ActorCriticRecurrent  # noqa: F401
from .ppo import PPO  # noqa: F401
from .rnd import RandomNetworkDistillation  # noqa: F401
from .rollout import RolloutStorage  # noqa: F401
from .runner import OnPolicyRunner  # noqa: F401
from .stairinfo import StairInfo  # noqa: F401
from .terrain_manager import TerrainManager  # noqa: F401
from .terrain_wells import build_stairwell_terrain, is_well_terrain_cfg  # noqa: F401
from .wells import WellScan  # noqa: F401

__all__ = ["Go2Env", "ActorCritic", "ActorCriticRecurrent", "RolloutStorage", "PPO", "RandomNetworkDistillation", "Distillation", "StudentTeacher", "StudentTeacherRecurrent", "distill_windows", "rdistill_schedule", "teacher_state_from_checkpoint", "OnPolicyRunner", "EmpiricalNormalization", "LidarScan", "StairInfo", "TerrainManager", "WellScan", "ContactTerms", "EvalStats", "Evaluator", "command_grid", "bin_metrics", "build_stairwell_terrain", "is_well_terrain_cfg", "init", "C", "Go2Sim", "Go2SimError", "load_hip_lib", "flatten_walk_cfg", "flatten_base_cfg", "get_walk_cfgs", "get_stair_cfgs", "get_rough_cfgs", "get_stairwell_cfgs", "get_stair_lidar_cfgs", "get_stair_info_cfg", "get_stair_info_cfgs",
           "get_crouch_cfgs", "get_jump_cfgs", "load_model_json", "pack_model", "load_cfgs", "save_cfgs", "read_checkpoint", "save_checkpoint", "allgather_records", "shard_envs", "shard_seed"]
