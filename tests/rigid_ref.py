"""Plain float64 rigid-body reference for the articulated dynamics (test helper, numpy only).

Independent of the library's formulation: no COM-frame spatial vectors, no cdof / cdofd.  Everything is in world coordinates, link by link:
link origins and rotations from the model tree, point Jacobians, the mass matrix as sum_i m_i Jv_i^T Jv_i + Jw_i^T I_i Jw_i, and the bias force
from a Newton-Euler pass at zero joint acceleration (angular velocity / acceleration and the acceleration of every link origin propagated down the
tree in closed form).

State conventions of the library (model_blob JSON): the free joint stores position then a wxyz quaternion; its linear velocity is in world axes and
its angular velocity in BODY axes; revolute joints rotate about `motion_ang` (link frame) by qpos - qpos0.
"""
import numpy as np

JOINT_REVOLUTE, JOINT_FREE = 1, 4
CTRL_FORCE, CTRL_VELOCITY, CTRL_POSITION = 0, 1, 2


def quat_to_mat(q):
    """Rotation matrix of a wxyz quaternion (normalised first)."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def mat_to_quat(R):
    """wxyz quaternion (w >= 0) of a rotation matrix."""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q if q[0] >= 0 else -q


def axis_angle(axis, theta):
    """Rodrigues rotation about a unit axis."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = skew(a)
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def quat_mul(u, v):
    w1, x1, y1, z1 = u
    w2, x2, y2, z2 = v
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def quat_exp(rv):
    """Unit quaternion of the rotation vector rv."""
    th = np.linalg.norm(rv)
    if th < 1e-300:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(0.5 * th)], np.sin(0.5 * th) * np.asarray(rv) / th])


class RigidRef:
    """The articulated robot of one model JSON in float64."""

    def __init__(self, model):
        self.m = model
        self.links, self.joints, self.dofs = model["links"], model["joints"], model["dofs"]
        self.nl, self.nd, self.nq = len(self.links), len(self.dofs), len(model["qpos0"])
        self.qpos0 = np.asarray(model["qpos0"], np.float64)
        self.gravity = np.asarray(model["gravity"], np.float64)
        self.dt = float(model["substep_dt"])
        self.armature = np.array([d["armature"] for d in self.dofs], np.float64)
        self.damping = np.array([d["damping"] for d in self.dofs], np.float64)
        self.stiffness = np.array([d["stiffness"] for d in self.dofs], np.float64)
        self.kp = np.array([d["kp"] for d in self.dofs], np.float64)
        self.kv = np.array([d["kv"] for d in self.dofs], np.float64)
        self.force_range = np.array([d["force_range"] for d in self.dofs], np.float64)
        self.limit = np.array([d["limit"] for d in self.dofs], np.float64)
        # the robot: links that move (a fixed link without dofs, e.g. the ground plane, has no Jacobian and takes no part)
        self.moving = [i for i, L in enumerate(self.links) if not L["is_fixed"]]
        self.root = self.moving[0] if self.moving else None

    def set_dof_gains(self, d, kp, kv, flo, fhi):
        self.kp[d], self.kv[d], self.force_range[d] = kp, kv, (flo, fhi)

    # ------------------------------------------------------------------------------------------------ kinematics
    def fk(self, qpos, qvel=None, mass_shift=None, com_shift=None):
        """World frames of every link.  Returns a dict with, per link l:
        R[l] (3x3), p[l] (origin), c[l] (centre of mass, com_shift applied in the link frame), mass[l] (mass_shift applied), I[l] (world inertia
        about the COM), and per dof d: ax[d] (world angular axis, 0 for translations), lin[d] (world linear direction, 0 for rotations), anc[d]
        (world point the axis passes through), link_of[d].  With qvel also w[l] (angular velocity), vo[l] (origin velocity), alpha[l] and ao[l]
        (angular acceleration and origin acceleration at zero joint acceleration, gravity excluded)."""
        qpos = np.asarray(qpos, np.float64)
        nl, nd = self.nl, self.nd
        mass_shift = np.zeros(nl) if mass_shift is None else np.asarray(mass_shift, np.float64)
        com_shift = np.zeros((nl, 3)) if com_shift is None else np.asarray(com_shift, np.float64).reshape(nl, 3)
        R = np.zeros((nl, 3, 3)); p = np.zeros((nl, 3)); c = np.zeros((nl, 3)); I = np.zeros((nl, 3, 3)); mass = np.zeros(nl)
        ax = np.zeros((nd, 3)); lin = np.zeros((nd, 3)); anc = np.zeros((nd, 3)); link_of = np.full(nd, -1)
        v = None if qvel is None else np.asarray(qvel, np.float64)
        w = np.zeros((nl, 3)); vo = np.zeros((nl, 3)); alpha = np.zeros((nl, 3)); ao = np.zeros((nl, 3))
        for l, L in enumerate(self.links):
            par = L["parent"]
            Rl = quat_to_mat(L["quat"]); pl = np.asarray(L["pos"], np.float64)
            wp = np.zeros(3); vp = np.zeros(3); alp = np.zeros(3); ap = np.zeros(3); pp = np.zeros(3)
            if par != -1:
                Rl = R[par] @ Rl; pl = p[par] + R[par] @ pl
                wp, alp, pp = w[par], alpha[par], p[par]
                vp = vo[par] + np.cross(w[par], pl - pp)                                   # velocity / acceleration of the (not yet moved) link origin
                ap = ao[par] + np.cross(alpha[par], pl - pp) + np.cross(w[par], np.cross(w[par], pl - pp))
            wl, vl, al, aol = wp.copy(), vp.copy(), alp.copy(), ap.copy()
            for j in range(L["joint_start"], L["joint_end"]):
                J = self.joints[j]
                ds, qs = J["dof_start"], J["q_start"]
                if J["type"] == JOINT_FREE:
                    pl = qpos[qs:qs + 3].copy()
                    Rl = quat_to_mat(qpos[qs + 3:qs + 7])
                    for i in range(3):
                        lin[ds + i, i] = 1.0; anc[ds + i] = pl; link_of[ds + i] = l
                        ax[ds + 3 + i] = Rl[:, i]; anc[ds + 3 + i] = pl; link_of[ds + 3 + i] = l
                    if v is not None:                     # world linear velocity, body angular velocity; at zero qacc both accelerations vanish
                        wl = Rl @ v[ds + 3:ds + 6]; vl = v[ds:ds + 3].copy(); al = np.zeros(3); aol = np.zeros(3)
                elif J["type"] == JOINT_REVOLUTE:
                    axis_l = np.asarray(self.dofs[ds]["motion_ang"], np.float64)
                    jpos = np.asarray(J["pos"], np.float64)
                    A = pl + Rl @ jpos                                                      # anchor: fixed in the parent and in the child
                    s = Rl @ axis_l
                    theta = qpos[qs] - self.qpos0[qs]
                    Rl = Rl @ axis_angle(axis_l, theta)
                    pl_new = A - Rl @ jpos
                    ax[ds] = s; anc[ds] = A; link_of[ds] = l
                    if v is not None:
                        qd = v[ds]
                        aA = aol + np.cross(al, A - pl) + np.cross(wl, np.cross(wl, A - pl))   # anchor as a point of the body before the joint
                        vA = vl + np.cross(wl, A - pl)
                        w_new = wl + s * qd
                        al = al + np.cross(wl, s) * qd                                      # d/dt (s qd) with s carried by the parent, qdd = 0
                        wl = w_new
                        vl = vA + np.cross(wl, pl_new - A)
                        aol = aA + np.cross(al, pl_new - A) + np.cross(wl, np.cross(wl, pl_new - A))
                    pl = pl_new
                else:
                    raise NotImplementedError("joint type %d" % J["type"])
            R[l], p[l] = Rl, pl
            w[l], vo[l], alpha[l], ao[l] = wl, vl, al, aol
            Ri = Rl @ quat_to_mat(L["inertial_quat"])
            c[l] = pl + Rl @ (np.asarray(L["inertial_pos"], np.float64) + com_shift[l])
            I[l] = Ri @ np.asarray(L["inertial_i"], np.float64) @ Ri.T
            mass[l] = L["inertial_mass"] + mass_shift[l]
        out = dict(R=R, p=p, c=c, I=I, mass=mass, ax=ax, lin=lin, anc=anc, link_of=link_of)
        if v is not None:
            out.update(w=w, vo=vo, alpha=alpha, ao=ao)
        mv = self.moving
        out["com"] = (mass[mv, None] * c[mv]).sum(0) / mass[mv].sum() if mv else np.zeros(3)
        return out

    def chain(self, l):
        """dofs that move link l (its own and its ancestors')."""
        ds = []
        while l != -1:
            L = self.links[l]
            ds.extend(range(L["dof_start"], L["dof_end"]))
            l = L["parent"]
        return sorted(ds)

    def jac(self, k, l, x):
        """(Jv, Jw): 3 x nd linear and angular Jacobians of the world point x moving with link l."""
        Jv = np.zeros((3, self.nd)); Jw = np.zeros((3, self.nd))
        x = np.asarray(x, np.float64)
        for d in self.chain(l):
            Jv[:, d] = k["lin"][d] + np.cross(k["ax"][d], x - k["anc"][d])
            Jw[:, d] = k["ax"][d]
        return Jv, Jw

    def point_vel(self, k, l, x):
        """Velocity of the point x of link l from the propagated origin velocity (independent of the Jacobian)."""
        return k["vo"][l] + np.cross(k["w"][l], np.asarray(x, np.float64) - k["p"][l])

    # ------------------------------------------------------------------------------------------------ dynamics
    def mass_matrix(self, k, ctrl_mode=None, implicit=True, extras=True):
        """M(q) = sum_i m_i Jv_i^T Jv_i + Jw_i^T I_i Jw_i (+ diag(armature) + dt diag(damping [+ kv in position / velocity mode]))."""
        M = np.zeros((self.nd, self.nd))
        for l in self.moving:
            Jv, Jw = self.jac(k, l, k["c"][l])
            M += k["mass"][l] * Jv.T @ Jv + Jw.T @ k["I"][l] @ Jw
        if extras:
            M += np.diag(self.armature)
            if implicit:
                kvd = self.damping.copy()
                if ctrl_mode is not None:
                    kvd = kvd + np.where((np.asarray(ctrl_mode) == CTRL_POSITION) | (np.asarray(ctrl_mode) == CTRL_VELOCITY), self.kv, 0.0)
                M += self.dt * np.diag(kvd)
        return M

    def bias(self, k, gravity=None):
        """c(q, v): Newton-Euler at zero joint acceleration, c = sum_i Jv_i^T m_i (a_i - g) + Jw_i^T (I_i alpha_i + w_i x I_i w_i)."""
        g = self.gravity if gravity is None else np.asarray(gravity, np.float64)
        cb = np.zeros(self.nd)
        for l in self.moving:
            r = k["c"][l] - k["p"][l]
            w, al = k["w"][l], k["alpha"][l]
            a = k["ao"][l] + np.cross(al, r) + np.cross(w, np.cross(w, r))
            Jv, Jw = self.jac(k, l, k["c"][l])
            Il = k["I"][l]
            cb += Jv.T @ (k["mass"][l] * (a - g)) + Jw.T @ (Il @ al + np.cross(w, Il @ w))
        return cb

    def kinetic_energy(self, k):
        T = 0.0
        for l in self.moving:
            vc = self.point_vel(k, l, k["c"][l])
            T += 0.5 * k["mass"][l] * vc @ vc + 0.5 * k["w"][l] @ k["I"][l] @ k["w"][l]
        return T

    def potential_energy(self, k):
        return -sum(k["mass"][l] * self.gravity @ k["c"][l] for l in self.moving)

    def momentum(self, k):
        """(linear momentum, angular momentum about the world origin)."""
        P = np.zeros(3); Lm = np.zeros(3)
        for l in self.moving:
            vc = self.point_vel(k, l, k["c"][l])
            P += k["mass"][l] * vc
            Lm += k["mass"][l] * np.cross(k["c"][l], vc) + k["I"][l] @ k["w"][l]
        return P, Lm

    def dof_pos(self, qpos):
        """qpos - qpos0 per revolute dof (the free joint's linear dofs: the position)."""
        out = np.zeros(self.nd)
        for J in self.joints:
            ds, qs = J["dof_start"], J["q_start"]
            if J["type"] == JOINT_FREE:
                out[ds:ds + 3] = qpos[qs:qs + 3]
            elif J["type"] == JOINT_REVOLUTE:
                out[ds] = qpos[qs] - self.qpos0[qs]
        return out

    def revolute_dofs(self):
        return [J["dof_start"] for J in self.joints if J["type"] == JOINT_REVOLUTE]

    def passive(self, qpos, qvel):
        """-damping v - stiffness (qpos - qpos0) (stiffness on revolute dofs only)."""
        f = -self.damping * np.asarray(qvel, np.float64)
        dp = self.dof_pos(qpos)
        for d in self.revolute_dofs():
            f[d] -= self.stiffness[d] * dp[d]
        return f

    def applied(self, qpos, qvel, ctrl_mode, ctrl_force=None, ctrl_pos=None, ctrl_vel=None):
        """Actuator force per dof, clamped to force_range: force mode ctrl_force, velocity mode kv (v* - v), position mode kp (q* - q) + kv (v* - v)
        (never on the free joint's angular dofs)."""
        nd = self.nd
        z = np.zeros(nd)
        cf = z if ctrl_force is None else np.asarray(ctrl_force, np.float64)
        cp = z if ctrl_pos is None else np.asarray(ctrl_pos, np.float64)
        cv = z if ctrl_vel is None else np.asarray(ctrl_vel, np.float64)
        v, dp = np.asarray(qvel, np.float64), self.dof_pos(qpos)
        free_ang = set()
        for J in self.joints:
            if J["type"] == JOINT_FREE:
                free_ang.update(range(J["dof_start"] + 3, J["dof_start"] + 6))
        f = np.zeros(nd)
        for d in range(nd):
            if ctrl_mode[d] == CTRL_FORCE:
                f[d] = cf[d]
            elif ctrl_mode[d] == CTRL_VELOCITY:
                f[d] = self.kv[d] * (cv[d] - v[d])
            elif ctrl_mode[d] == CTRL_POSITION and d not in free_ang:
                f[d] = self.kp[d] * (cp[d] - dp[d]) + self.kv[d] * (cv[d] - v[d])
        return np.clip(f, self.force_range[:, 0], self.force_range[:, 1])

    def external(self, k, forces):
        """Generalised force of world forces applied at link origins: sum_l J_origin(l)^T f_l.  forces: {link: f}."""
        out = np.zeros(self.nd)
        for l, f in forces.items():
            Jv, _ = self.jac(k, l, k["p"][l])
            out += Jv.T @ np.asarray(f, np.float64)
        return out

    # ------------------------------------------------------------------------------------------------ integration
    def qdot(self, qpos, qvel):
        """d qpos / dt: world linear velocity, 0.5 quat (x) (0, w_body), revolute v."""
        qd = np.zeros(self.nq)
        for J in self.joints:
            ds, qs = J["dof_start"], J["q_start"]
            if J["type"] == JOINT_FREE:
                qd[qs:qs + 3] = qvel[ds:ds + 3]
                qd[qs + 3:qs + 7] = 0.5 * quat_mul(qpos[qs + 3:qs + 7], np.concatenate([[0.0], qvel[ds + 3:ds + 6]]))
            elif J["type"] == JOINT_REVOLUTE:
                qd[qs] = qvel[ds]
        return qd

    def integrate(self, qpos, qvel, acc):
        """Semi-implicit Euler: v' = v + a dt, p' = p + v' dt, quat' = normalise(quat (x) exp(w'_body dt)), revolute q' = q + v' dt."""
        dt = self.dt
        v1 = np.asarray(qvel, np.float64) + np.asarray(acc, np.float64) * dt
        q1 = np.asarray(qpos, np.float64).copy()
        for J in self.joints:
            ds, qs = J["dof_start"], J["q_start"]
            if J["type"] == JOINT_FREE:
                q1[qs:qs + 3] = q1[qs:qs + 3] + v1[ds:ds + 3] * dt
                qn = quat_mul(q1[qs + 3:qs + 7], quat_exp(v1[ds + 3:ds + 6] * dt))
                q1[qs + 3:qs + 7] = qn / np.linalg.norm(qn)
            elif J["type"] == JOINT_REVOLUTE:
                q1[qs] = q1[qs] + v1[ds] * dt
        return q1, v1

    # ------------------------------------------------------------------------------------------------ constraints
    @staticmethod
    def orthogonals(a):
        """The two tangent directions of a contact normal (Genesis geom.py `orthogonals`)."""
        a = np.asarray(a, np.float64)
        if abs(a[1]) < 0.5:
            b = np.array([-a[0] * a[1], 1.0 - a[1] * a[1], -a[2] * a[1]])
        else:
            b = np.array([-a[0] * a[2], -a[1] * a[2], 1.0 - a[2] * a[2]])
        b = b / np.linalg.norm(b)
        return b, np.cross(a, b)

    def contact_rows(self, k, link_a, link_b, pos, normal, mu):
        """The 4 pyramid rows of one contact: row_i . v = (v_b(pos) - v_a(pos)) . (+-mu d_k - n), and the 4 directions."""
        d1, d2 = self.orthogonals(normal)
        n = np.asarray(normal, np.float64)
        Ja = self.jac(k, link_a, pos)[0] if link_a >= 0 else np.zeros((3, self.nd))
        Jb = self.jac(k, link_b, pos)[0] if link_b >= 0 else np.zeros((3, self.nd))
        rows, dirs = [], []
        for i in range(4):
            d = (2 * (i % 2) - 1) * (d1 if i < 2 else d2)
            dirn = mu * d - n
            rows.append((Jb - Ja).T @ dirn)
            dirs.append(dirn)
        return np.array(rows), np.array(dirs)

    def limit_rows(self, qpos, limit=None):
        """Rows of the violated joint limits in joint order: +1 below the lower limit, -1 above the upper one (limit: other bounds than the
        model's float64 ones, e.g. the float32 numbers the library stores)."""
        rows = []
        limit = self.limit if limit is None else limit
        for J in self.joints:
            if J["type"] != JOINT_REVOLUTE:
                continue
            d, q = J["dof_start"], qpos[J["q_start"]]
            lo, hi = q - limit[d, 0], limit[d, 1] - q
            if min(lo, hi) < 0:
                r = np.zeros(self.nd)
                r[d] = 1.0 if lo < hi else -1.0
                rows.append(r)
        return np.array(rows).reshape(-1, self.nd)

    def inverse_weights(self):
        """Inverse weights at qpos0 with M = inertia + armature (no damping term): per link the means of the translational and of the rotational
        diagonal of J M^-1 J^T (J at the link's centre of mass), per dof the diagonal of M^-1 (a free joint: averaged over its three translations
        and over its three rotations), and the mean inertia trace(M) / nd."""
        k = self.fk(self.qpos0)
        M = self.mass_matrix(k, implicit=False)
        Minv = np.linalg.inv(M)
        link = np.zeros((self.nl, 2))
        for l in range(self.nl):
            Jv, Jw = self.jac(k, l, k["c"][l])
            link[l] = np.diag(Jv @ Minv @ Jv.T).mean(), np.diag(Jw @ Minv @ Jw.T).mean()
        dof = np.diag(Minv).copy()
        for J in self.joints:
            if J["type"] == JOINT_FREE:
                ds = J["dof_start"]
                dof[ds:ds + 3] = dof[ds:ds + 3].mean()
                dof[ds + 3:ds + 6] = dof[ds + 3:ds + 6].mean()
        return link, dof, np.trace(M) / self.nd

    def contact_params(self, geom_a, geom_b, friction, ratio):
        """(mu, the seven solver parameters, inverse weight) of a contact between two geoms.  friction, ratio: per-geom arrays of one env.
        mu = max(friction_a ratio_a, friction_b ratio_b, 0.01); the solver parameters are the mean of the two geoms'; the inverse weight is the
        sum of the two links' translational inverse weights (a fixed link such as the ground has none).  The model's values are taken as the
        float32 numbers the library stores."""
        ga, gb = self.m["geoms"][geom_a], self.m["geoms"][geom_b]
        mu = max(float(friction[geom_a]) * float(ratio[geom_a]), float(friction[geom_b]) * float(ratio[geom_b]), 0.01)
        sol = 0.5 * (_f32(ga["sol_params"]) + _f32(gb["sol_params"]))
        w = sum(float(_f32(self.links[g["link"]]["invweight"][0])) for g in (ga, gb) if not self.links[g["link"]]["is_fixed"])
        return mu, sol, w

    def constraint_problem(self, k, qpos, vel, contacts, friction, ratio):
        """The constraint rows of one env at the start of a substep.  k: fk() of the state, qpos / vel: the state (vel: the velocity the substep
        starts from), contacts: a list of (geom_a, geom_b, pos, normal, penetration) in the library's order, friction / ratio: per-geom arrays.
        Rows: four per contact in contact order, then one per violated joint limit in joint order.  Returns a dict with J (n x nd), aref, D = 1 / diag,
        imp, branch (BRANCH_*), and is_limit per row."""
        eps = float(_f32(self.m["eps"]))
        vel = np.asarray(vel, np.float64)
        J, aref, D, imp, branch, is_limit = [], [], [], [], [], []
        for ga, gb, pos, normal, pen in contacts:
            mu, sol, w = self.contact_params(ga, gb, friction, ratio)
            rows, _ = self.contact_rows(k, self.m["geoms"][ga]["link"], self.m["geoms"][gb]["link"], pos, normal, mu)
            for r in rows:
                im, ar, br = imp_aref(sol, -float(pen), r @ vel)
                J.append(r); aref.append(ar); imp.append(im); branch.append(br); is_limit.append(False)
                D.append(1.0 / max((w + mu * mu * w) * 2.0 * mu * mu * (1.0 - im) / im, eps))
        lim32 = _f32(self.limit)
        for r in self.limit_rows(qpos, lim32):
            d = int(np.flatnonzero(r)[0])
            joint = next(Jn for Jn in self.joints if Jn["dof_start"] == d)
            q = float(qpos[joint["q_start"]])
            delta = min(q - lim32[d, 0], lim32[d, 1] - q)
            im, ar, br = imp_aref(_f32(joint["sol_params"]), delta, r @ vel)
            J.append(r); aref.append(ar); imp.append(im); branch.append(br); is_limit.append(True)
            D.append(1.0 / max(float(_f32(self.dofs[d]["invweight"])) * (1.0 - im) / im, eps))
        return dict(J=np.array(J).reshape(-1, self.nd), aref=np.array(aref), D=np.array(D), imp=np.array(imp), branch=np.array(branch, int),
                    is_limit=np.array(is_limit, bool))


def _f32(x):
    """x as the library holds it: rounded to float32, returned in float64."""
    return np.asarray(x, np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- the constraint law
BRANCH_LOW, BRANCH_HIGH, BRANCH_SAT = 0, 1, 2      # x = |pos| / width below mid, between mid and 1, beyond 1


def impedance(sol, pos):
    """(impedance, branch) at the constraint position pos (contacts: minus the penetration, limits: the violation) from the solver parameters
    (timeconst, dampratio, dmin, dmax, width, mid, power): with x = |pos| / width and the unit curve y(x) = x^p / mid^(p-1) below mid,
    1 - (1 - x)^p / (1 - mid)^(p-1) from mid to 1, the impedance is dmin + y (dmax - dmin) kept within [dmin, dmax], and dmax beyond x = 1."""
    _, _, dmin, dmax, width, mid, power = (float(v) for v in sol)
    x = abs(float(pos)) / width
    if x > 1.0:
        return dmax, BRANCH_SAT
    if x < mid:
        y, branch = x ** power / mid ** (power - 1.0), BRANCH_LOW
    else:
        y, branch = 1.0 - (1.0 - x) ** power / (1.0 - mid) ** (power - 1.0), BRANCH_HIGH
    return min(max(dmin + y * (dmax - dmin), dmin), dmax), branch


def imp_aref(sol, pos, vel):
    """(impedance, reference acceleration, branch) of one row: aref = -b vel - k imp pos, the critically-scaled spring-damper with
    b = 2 / (dmax timeconst) and k = 1 / (dmax timeconst dampratio)^2."""
    timeconst, dampratio, _, dmax = (float(v) for v in sol[:4])
    imp, branch = impedance(sol, pos)
    b = 2.0 / (dmax * timeconst)
    kk = 1.0 / (dmax * timeconst * dampratio) ** 2
    return imp, -b * float(vel) - kk * imp * float(pos), branch


def constraint_cost(M, a0, J, aref, D, a):
    """1/2 (a - a0)^T M (a - a0) + 1/2 sum_i D_i min(0, (J a - aref)_i)^2."""
    r = np.minimum(J @ a - aref, 0.0)
    return 0.5 * (a - a0) @ M @ (a - a0) + 0.5 * (D * r) @ r


def constraint_force(J, aref, D, a):
    """The force of every row at the acceleration a: D_i max(0, -(J a - aref)_i)."""
    return D * np.maximum(0.0, -(J @ a - aref))


def solve_constraints(M, a0, J, aref, D, rtol=1e-10, max_iter=200):
    """The minimiser of constraint_cost, a strictly convex piecewise quadratic: Newton on the active set (J a - aref)_i < 0 with a backtracking line
    search, until the gradient is below rtol of the force scale max(|M| |a0| + |J|^T D (|J| |a0| + |aref|)).  Returns (a, cost, active set,
    max |gradient| / force scale)."""
    a = np.array(a0, np.float64)
    fscale = (np.abs(M) @ np.abs(a0) + np.abs(J).T @ (D * (np.abs(J) @ np.abs(a0) + np.abs(aref)))).max() + 1e-300
    cost = constraint_cost(M, a0, J, aref, D, a)
    for _ in range(max_iter):
        active = J @ a - aref < 0.0
        g = M @ (a - a0) - J.T @ constraint_force(J, aref, D, a)
        if np.abs(g).max() <= rtol * fscale:
            break
        Ja = J[active]
        step = -np.linalg.solve(M + Ja.T @ (D[active, None] * Ja), g)
        t = 1.0
        while True:
            c1 = constraint_cost(M, a0, J, aref, D, a + t * step)
            if c1 <= cost + 1e-4 * t * (g @ step) or t < 1e-12:
                break
            t *= 0.5
        a, cost = a + t * step, c1
    else:
        raise RuntimeError("solve_constraints: no convergence")
    return a, cost, active, np.abs(g).max() / fscale
