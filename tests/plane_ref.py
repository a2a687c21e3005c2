"""A numpy float64 restatement of the narrow phase against the infinite ground plane (gs.morphs.Plane), independent of the library's code.

Semantics (the reference's collider):
  * plane vs sphere / cylinder: the plane branch of func_convex_convex_contact (narrowphase.py:659-678) inside the 5-detection perturbation loop
    (:613-900): normal = -(R_a data[0:3]) normalised, one support point v1 of b along it, penetration = normal . (v1 - pos_a), contact at
    v1 - penetration / 2 * normal; the perturbed detections (multi-contact unless b is a sphere) rotate both frames about the first contact, and their
    contacts get the position / normal correction, the de-duplication against the pair's earlier contacts and the `penetration > -tolerance` test;
  * plane vs box: func_plane_box_contact (box_contact.py:25-93), a pass of its own after every convex-convex contact: the deepest corner, then the
    corners in vertex order while the pair has fewer than n_contacts_per_pair contacts, each kept if it penetrates and lies more than `tolerance`
    from the first contact;
  * func_compute_tolerance / func_contact_orthogonals with a plane as geom a (contact.py:265-345): only b's AABB size counts, b is the reference
    geometry.
  * broad phase: a pair exists when the geom's AABB (its init-AABB corners moved to the world) overlaps the plane's; pairs are ordered by the lower
    x-end of the geom's AABB (the sweep key of the plane pair: the plane's x-min comes first of all endpoints).

Cylinders use the model's support table exactly as the reference's support field does (support_field.py:138-180: the 180 x 180 direction grid, whose
cells the compiled model stores as a theta -> rim-vertex map and the 32-gon rim).

Every keep / drop decision records its distance to the threshold in `margin` (penetration vs 0, corner distance vs tolerance, de-duplication
distance, `> -tolerance`, grid cell edges of the cylinder table, ties between support candidates, the orthogonals' axis choice, AABB overlaps and
the pair order), so that a test can draw states on which float32 and float64 make the same decisions."""
import numpy as np

GEOM_PLANE, GEOM_SPHERE, GEOM_CYLINDER, GEOM_BOX = 0, 1, 3, 5


def quat_mul(u, v):
    w1, x1, y1, z1 = u
    w2, x2, y2, z2 = v
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def quat_to_R(q):
    q = np.asarray(q, np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def inv_quat(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def rotvec_to_quat(rv):
    th = np.linalg.norm(rv)
    if th == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(0.5 * th)], np.sin(0.5 * th) / th * np.asarray(rv)])


def rotate_frame(pos, quat, contact_pos, qrot):
    """func_rotate_frame, contact.py:348-369."""
    q = quat_mul(qrot, quat)
    rel = contact_pos - pos
    return pos - (quat_to_R(qrot) @ rel - rel), q / np.linalg.norm(q)


class PlaneRef:
    def __init__(self, model):
        self.m = model
        self.geoms = model["geoms"]
        self.links = model["links"]
        col = model["collider"]
        self.mc_perturbation, self.mc_tolerance = col["mc_perturbation"], col["mc_tolerance"]
        self.n_contacts_per_pair = col["n_contacts_per_pair"]
        self.theta_to_ring = np.asarray(model["support_theta_to_ring"])
        assert self.geoms[0]["type"] == GEOM_PLANE, "the model's ground is not a plane (model_blob.with_plane_ground)"
        self.margin = np.inf

    def _note(self, d):
        self.margin = min(self.margin, abs(float(d)))

    # ---- poses -------------------------------------------------------------------------------------------------------
    def geom_poses(self, link_pos, link_quat):
        """World poses of every geom from the link poses: pos = p_l + R_l g.pos, quat = q_l * g.quat."""
        gp, gq = [], []
        for g in self.geoms:
            l = g["link"]
            R = quat_to_R(link_quat[l])
            gp.append(np.asarray(link_pos[l], np.float64) + R @ np.asarray(g["pos"], np.float64))
            q = quat_mul(np.asarray(link_quat[l], np.float64), np.asarray(g["quat"], np.float64))
            gq.append(q / np.linalg.norm(q))
        return np.array(gp), np.array(gq)

    def inertial_quat(self, link_quat, l):
        q = quat_mul(np.asarray(link_quat[l], np.float64), np.asarray(self.links[l]["inertial_quat"], np.float64))
        return q / np.linalg.norm(q)

    def aabb(self, i_g, pos, quat):
        c = np.asarray(self.geoms[i_g]["init_aabb"], np.float64) @ quat_to_R(quat).T + pos
        return c.min(0), c.max(0)

    # ---- support functions -------------------------------------------------------------------------------------------
    def support_cylinder_local(self, g, d):
        """_func_support_mesh on the cylinder's support field (support_field.py:138-180)."""
        theta = np.arctan2(d[1], d[0])
        phi = np.arccos(np.clip(d[2], -1.0, 1.0))
        ii = (theta + np.pi) / np.pi / 2.0 * 180.0
        jj = phi / np.pi * 180.0
        for x in (ii, jj, jj - 90.0):
            self._note(x - np.round(x))
        wrap = lambda x: 0 if not x >= 0 else min(int(x - 180) if x >= 180 else int(x), 179)
        clampi = lambda x: 0 if not x >= 0 else (179 if x >= 179 else int(x))
        i_lo, i_hi = wrap(np.floor(ii)), wrap(np.ceil(ii))
        j_lo = clampi(np.floor(jj)); j_lo = 1 if j_lo == 0 else j_lo
        j_hi = clampi(np.ceil(jj)); j_hi = 178 if j_hi == 179 else j_hi
        rim, half = np.asarray(g["rim"], np.float64), 0.5 * g["data"][1]
        cands = []
        for i4 in range(4):
            hi_i, hi_j = i4 % 2 != 0, i4 // 2 > 0
            k = self.theta_to_ring[i_hi if hi_i else i_lo]
            j = j_hi if hi_j else j_lo
            cands.append(np.array([rim[k][0], rim[k][1], half if j <= 90 else -half]))
        dots = [float(c @ d) for c in cands]
        best = int(np.argmax(dots))                                            # the first maximum, like the strict `>` of the loop
        for c, dt in zip(cands, dots):
            if not np.array_equal(c, cands[best]):
                self._note(dots[best] - dt)
        return cands[best]

    def support(self, i_g, d, pos, quat):
        g = self.geoms[i_g]
        t = g["type"]
        if t == GEOM_SPHERE:
            return pos + d * g["data"][0]
        R = quat_to_R(quat)
        dl = R.T @ d
        if t == GEOM_BOX:
            for x in dl:
                self._note(x)
            return R @ (np.where(dl < 0.0, -1.0, 1.0) * 0.5 * np.asarray(g["data"][:3], np.float64)) + pos
        if t == GEOM_CYLINDER:
            return R @ self.support_cylinder_local(g, dl) + pos
        raise ValueError("no support function for geom type %d" % t)

    # ---- contact.py ----------------------------------------------------------------------------------------------------
    def tolerance(self, i_gb):
        a = np.asarray(self.geoms[i_gb]["init_aabb"], np.float64)
        return 0.5 * self.mc_tolerance * np.linalg.norm(a[7] - a[0])

    def orthogonals(self, i_gb, normal, link_quat):
        rot = quat_to_R(self.inertial_quat(link_quat, self.geoms[i_gb]["link"]))
        ang = np.abs(rot.T @ normal)
        order = np.argsort(-ang, kind="stable")
        self._note(ang[order[0]] - ang[order[1]])
        idx = (int(order[0]) + 1) % 3
        a0 = rot[:, idx]
        a0 = a0 - normal.dot(a0) * normal
        a0 = a0 / np.linalg.norm(a0)
        return a0, np.cross(normal, a0)

    # ---- narrow phase ----------------------------------------------------------------------------------------------------
    def plane_normal(self, plane_quat):
        n = quat_to_R(plane_quat) @ np.asarray(self.geoms[0]["data"][:3], np.float64)
        return -n / np.linalg.norm(n)

    def plane_contact(self, i_gb, pa, qa, pb, qb):
        normal = self.plane_normal(qa)
        v1 = self.support(i_gb, normal, pb, qb)
        pen = float(normal @ (v1 - pa))
        self._note(pen)
        return pen > 0.0, normal, v1 - 0.5 * pen * normal, pen

    def convex_pair(self, i_gb, gp, gq, link_quat):
        """func_convex_convex_contact for (plane, b): list of (normal, pos, penetration)."""
        out = []
        multi = self.geoms[i_gb]["type"] != GEOM_SPHERE
        tol = self.tolerance(i_gb)
        pa0, qa0, pb0, qb0 = gp[0], gq[0], gp[i_gb], gq[i_gb]
        is_col0, normal0, cpos0, pen0 = self.plane_contact(i_gb, pa0, qa0, pb0, qb0)
        if not is_col0:
            return out
        out.append((normal0, cpos0, pen0))
        if not multi:
            return out
        ax0, ax1 = self.orthogonals(i_gb, normal0, link_quat)
        eps = self.mc_perturbation
        for i_det in range(1, 5):
            axis = (2 * (i_det % 2) - 1) * ax0 + (1 - 2 * ((i_det // 2) % 2)) * ax1
            qrot = rotvec_to_quat(eps * axis)
            pa, qa = rotate_frame(pa0, qa0, cpos0, qrot)
            pb, qb = rotate_frame(pb0, qb0, cpos0, inv_quat(qrot))
            is_col, normal, cpos, pen = self.plane_contact(i_gb, pa, qa, pb, qb)
            if not is_col:
                continue
            Rq = quat_to_R(qrot)
            cpa = Rq.T @ ((cpos - 0.5 * pen * normal) - cpos0) + cpos0
            cpb = Rq @ ((cpos + 0.5 * pen * normal) - cpos0) + cpos0
            cpos = 0.5 * (cpa + cpb)
            tw = np.cross(normal, normal0)
            for x in tw:
                self._note(abs(x) - eps)
            normal = normal + np.cross(np.clip(tw, -eps, eps), normal)
            pen = float(normal @ (cpb - cpa))
            repeated = False
            for prev in out:
                dist = np.linalg.norm(cpos - prev[1])
                self._note(dist - tol)
                if dist < tol:
                    repeated = True
            if repeated:
                continue
            self._note(pen + tol)
            if pen > -tol:
                out.append((normal, cpos, max(pen, 0.0)))
        return out

    def plane_box(self, i_gb, gp, gq):
        """func_plane_box_contact: list of (normal, pos, penetration)."""
        g = self.geoms[i_gb]
        normal = self.plane_normal(gq[0])
        v1 = self.support(i_gb, normal, gp[i_gb], gq[i_gb])
        pen0 = float(normal @ (v1 - gp[0]))
        self._note(pen0)
        if not pen0 > 0.0:
            return []
        cpos0 = v1 - 0.5 * pen0 * normal
        out = [(normal, cpos0, pen0)]
        tol = self.tolerance(i_gb)
        R = quat_to_R(gq[i_gb])
        for c in np.asarray(g["init_aabb"], np.float64):
            if len(out) >= self.n_contacts_per_pair:
                break
            corner = R @ c + gp[i_gb]
            pen = float(normal @ (corner - gp[0]))
            self._note(pen)
            if pen > 0.0:
                cpos = corner - 0.5 * pen * normal
                dist = np.linalg.norm(cpos - cpos0)
                self._note(dist - tol)
                if dist > tol:
                    out.append((normal, cpos, pen))
        return out

    def broad_pairs(self, gp, gq, robot_geoms):
        """Geoms whose AABB overlaps the plane's, in sweep order (ascending lower x-end)."""
        plo, phi = self.aabb(0, gp[0], gq[0])
        keep = []
        for i_g in robot_geoms:
            lo, hi = self.aabb(i_g, gp[i_g], gq[i_g])
            seps = np.concatenate([phi - lo, hi - plo])                            # overlap iff all > 0
            for x in seps:
                self._note(x)
            if np.all(seps > 0.0):
                keep.append((lo[0], i_g))
        keep.sort()
        return [i for _, i in keep], [x for x, _ in keep]

    def contacts(self, link_pos, link_quat, robot_geoms):
        """The contact list of one collision pass: [(geom_a, geom_b, normal, pos, penetration)], convex-convex pairs first, then plane-box pairs,
        each pass in broad-phase order.  `robot_geoms`: the geoms that the model pairs with the ground."""
        self.margin = np.inf
        gp, gq = self.geom_poses(link_pos, link_quat)
        order, xmin = self.broad_pairs(gp, gq, robot_geoms)
        convex, boxes = [], []
        for i_g, x in zip(order, xmin):
            if self.geoms[i_g]["type"] == GEOM_BOX:
                boxes.append((i_g, x, self.plane_box(i_g, gp, gq)))
            else:
                convex.append((i_g, x, self.convex_pair(i_g, gp, gq, link_quat)))
        out = []
        for group in (convex, boxes):
            xs = [x for _, x, cs in group if cs]
            for a, b in zip(xs[:-1], xs[1:]):                                     # the order of the pairs that produce contacts
                self.margin = min(self.margin, 10.0 * abs(b - a))
            for i_g, _, cs in group:
                out += [(0, i_g, n, p, d) for n, p, d in cs]
        return out
