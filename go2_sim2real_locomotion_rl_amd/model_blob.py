"""Packs the compiled Go2 model tables (model/go2_model.json) into the binary "GO2M" v1 blob that
`go2sim_create` consumes.  The layout is documented in include/go2sim.h."""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_JSON = os.path.join(_HERE, "model", "go2_model.json")
MAGIC = 0x4D324F47
VERSION = 1


def load_model_json(path=MODEL_JSON):
    with open(path) as f:
        return json.load(f)


def pack_model(model=None):
    m = load_model_json() if model is None else model
    F, I = [], []
    sol, col = m["solver"], m["collider"]
    F += [m["substep_dt"], *m["gravity"], m["eps"], sol["tolerance"], sol["ls_tolerance"], m["meaninertia"],
          col["mc_perturbation"], col["mc_tolerance"], col["mpr_to_gjk_overlap_ratio"], col["ccd_eps"],
          col["ccd_tolerance"], 0.0, 0.0, 0.0]
    for l in m["links"]:
        F += [*l["pos"], *l["quat"], *l["inertial_pos"], *l["inertial_quat"],
              *np.asarray(l["inertial_i"]).reshape(-1).tolist(), l["inertial_mass"], *l["invweight"]]
        I += [l["parent"], l["root"], l["entity"], l["is_fixed"], l["joint_start"], l["joint_end"], l["dof_start"],
              l["dof_end"], l["q_start"], l["q_end"], l["n_dofs"], l["geom_start"], l["geom_end"]]
    for j in m["joints"]:
        F += [*j["pos"], *j["sol_params"]]
        I += [j["type"], j["link"], j["q_start"], j["dof_start"], j["dof_end"]]
    for d in m["dofs"]:
        F += [*d["motion_ang"], *d["motion_vel"], *d["limit"], d["invweight"], d["armature"], d["damping"],
              d["stiffness"], d["frictionloss"], d["kp"], d["kv"], *d["force_range"]]
    F += list(m["qpos0"])
    for g in m["geoms"]:
        rim = np.zeros((32, 2))
        if g["rim"]:
            rim[:] = np.asarray(g["rim"])
        F += [*g["pos"], *g["quat"], *g["data"], g["friction"], *g["sol_params"], *g["center"],
              *np.asarray(g["init_aabb"]).reshape(-1).tolist(), *rim.reshape(-1).tolist()]
        I += [g["type"], g["link"], g["is_convex"]]
    F += list(m["mass_parent_mask"])
    for e in m["entities"]:
        I += [e["link_start"], e["link_end"], e["dof_start"], e["dof_end"], e["geom_start"], e["geom_end"]]
    I += list(m["collision_pair_idx"])
    I += list(m["support_theta_to_ring"])
    Fa = np.asarray(F, dtype=np.float32)
    Ia = np.asarray(I, dtype=np.int32)
    H = np.zeros(32, dtype=np.int32)
    H[:20] = [MAGIC, VERSION, len(m["links"]), len(m["joints"]), len(m["dofs"]), len(m["qpos0"]), len(m["geoms"]),
              len(m["entities"]), m["n_possible_pairs"], col["max_collision_pairs"], col["max_contact_pairs"],
              col["max_broad_pairs"], col["n_contacts_per_pair"], sol["iterations"], sol["ls_iterations"],
              col["ccd_iterations"], 180, 32, Fa.size, Ia.size]
    return H.tobytes() + Fa.tobytes() + Ia.tobytes()


GEOM_PLANE = 0
PLANE_THICKNESS = 1e-2     # utils/mesh.py create_plane: the collision box under the plane ("for safety")


def _z_up_to_R(z, eps=float(np.finfo(np.float32).eps)):
    """genesis/utils/geom.py _np_z_up_to_R without `up`: the rotation whose third column is the unit vector along z."""
    z = np.asarray(z, np.float64)
    n = np.linalg.norm(z)
    z = z / n if n > eps else np.array([0.0, 1.0, 0.0])
    x = np.array([z[1], -z[0], 0.0]) if abs(z[2]) < 1.0 - eps else np.array([z[2], 0.0, -z[0]])
    xn = np.linalg.norm(x)
    if not xn > eps:
        return np.eye(3)
    x = x / xn
    return np.stack([x, np.cross(z, x), z], axis=1)


def plane_init_aabb(normal=(0.0, 0.0, 1.0), plane_size=(1e3, 1e3)):
    """The 8 init-AABB corners of a gs.morphs.Plane geom (x slowest, z fastest; abd/misc.py:502-509): the bounding box of its collision mesh, a
    plane_size[0] x plane_size[1] x 1 cm box whose top face lies on the plane, turned to the normal (utils/mesh.py create_plane)."""
    hx, hy = 0.5 * float(plane_size[0]), 0.5 * float(plane_size[1])
    verts = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-PLANE_THICKNESS, 0.0)])
    verts = verts @ _z_up_to_R(normal).T
    lo, hi = verts.min(0), verts.max(0)
    return [[float((hi if i & 4 else lo)[0]), float((hi if i & 2 else lo)[1]), float((hi if i & 1 else lo)[2])] for i in range(8)]


def with_plane_ground(model, pos=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0), plane_size=(1e3, 1e3)):
    """A copy of a compiled model whose ground (geom 0 on the fixed link 0) is the infinite plane of gs.morphs.Plane (rigid_entity.py:366-376): geom
    type 0, data[0:3] = the unit normal in the geom frame, the link at `pos`, and the init AABB of the plane's finite collision box (plane_init_aabb),
    which is what the broad phase sees.  Link, geom and pair counts are unchanged, so the model runs on the library it was compiled for."""
    import copy

    n = np.asarray(normal, np.float64)
    if n.shape != (3,) or not np.linalg.norm(n) > 0.0:
        raise ValueError("normal must be a non-zero 3-vector")
    n = n / np.linalg.norm(n)                                                        # options/morphs.py Plane.__init__
    m = copy.deepcopy(model)
    g = m["geoms"][0]
    if g["link"] != 0 or not m["links"][0]["is_fixed"]:
        raise ValueError("geom 0 must be the ground geom on the fixed link 0")
    aabb = plane_init_aabb(n, plane_size)
    g["type"] = GEOM_PLANE
    g["data"] = [float(n[0]), float(n[1]), float(n[2]), 0.0, 0.0, 0.0, 0.0]
    g["pos"], g["quat"] = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]
    g["init_aabb"] = aabb
    g["center"] = [0.5 * (aabb[0][k] + aabb[7][k]) for k in range(3)]
    g["rim"] = None
    g["is_convex"] = 1
    m["links"][0]["pos"] = [float(v) for v in pos]
    m["links"][0]["quat"] = [1.0, 0.0, 0.0, 0.0]
    return m
