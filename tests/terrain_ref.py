"""A numpy float64 restatement of the heightfield narrow phase (gs.morphs.Terrain), independent of the library's code.

Semantics (the reference's collider):
  * heightfield: collider.py:374-394: heights hf * vertical_scale, terrain_xyz_maxmin = [rows * hs, cols * hs, hmax, 0, 0, hmin - 1]; the heightfield's
    geom sits at the terrain origin, unrotated, and its init AABB spans [0, (rows - 1) hs] x [0, (cols - 1) hs] x [hmin - 1, hmax];
  * pairs: the geoms paired with the ground whose AABB overlaps the heightfield's.  func_narrow_phase_any_vs_terrain (narrowphase.py:1197-1244) runs
    after every convex-convex contact, in broad-phase order: the sweep (broadphase.py:141-396) emits (geom, heightfield) at the later of the two lower
    x-ends, so the terrain pairs come out in ascending lower x-end of the geom's AABB;
  * per pair, func_contact_mpr_terrain (narrowphase.py:345-490): the geom's pose moved into the heightfield's frame, its bounding box from six support
    points, the early return when that box misses terrain_xyz_maxmin, the cell range floor / ceil with its clamps, then the vertex walk over rows
    r_min <= r < r_max, columns c_min <= c <= c_max, vertex i = 0, 1 (func_add_prism_vert, :493-512: x = hs (r + i), y = hs c, z = hf[r + i, c]).
    Once a row has pushed three vertices, the triangular prism of the last three (bottoms at hmin - 1) is tested with MPR if one of its top vertices
    is >= the geom's lowest point.  The walk stops once the pair holds n_contacts_per_pair contacts;
  * MPR: func_mpr_contact_from_centers (mpr.py:686-765) from the geom's centre and the prism's centroid: mpr_discover_portal (:445-598),
    mpr_refine_portal (:232-278), mpr_find_penetration (:338-423, the branch without MuJoCo compatibility: depth = portal normal . v1, normal = -portal
    normal), mpr_find_pos (:281-316, the same branch: barycentric weights of the portal along its normal; it has no inside tests or segment clamps)
    and mpr_expand_portal (:426-442), with the model's CCD_EPS, CCD_TOLERANCE and iteration cap;
  * a contact is kept unless it lies within func_compute_tolerance (contact.py:265-283: half of mc_tolerance times the smaller init-AABB diagonal of
    the two geoms) of one of the pair's earlier contacts;
  * _func_support_prism (support_field.py:265-282): the top vertices if d_z >= 0, the bottom ones otherwise, the first maximum.
Sphere / box / cylinder supports are tests/plane_ref.py's (the cylinder through the model's 180 x 180 support table).

Every keep / drop decision records its distance to the threshold in `margin`: the CCD_EPS sign tests of the portal search and refinement, the refine
stop rule, the iteration cap (margin 0 when hit), the choice of the portal vertex to replace, support argmax ties (prism vertices and box / cylinder
supports), the cylinder table's cell edges, the AABB overlap with the heightfield, the early return, the cell range floor / ceil, the eligibility of a
prism, the de-duplication distance and the pair order.  Distances are divided by the float32 rounding unit at the pair's coordinates (2^-24 times
the largest terrain-frame or world coordinate of the geom, at least 1 m): terrain-frame x and y reach 35 m and 78 m on the stair field, where one
float32 ulp is several um, larger than CCD_TOLERANCE.  A test that keeps the poses whose margin exceeds some hundreds of units draws states on which
float32 and float64 make the same decisions."""
import numpy as np

from plane_ref import PlaneRef, quat_to_R

F32_UNIT = 2.0 ** -24


def unit(v):
    return v / np.linalg.norm(v)


def add_prism_vert(prism, x, y, z):
    """func_add_prism_vert, narrowphase.py:493-512: shift the strip by one vertex; the bottoms keep their height."""
    prism[0], prism[1], prism[3], prism[4] = prism[1].copy(), prism[2].copy(), prism[4].copy(), prism[5].copy()
    prism[2][0] = prism[5][0] = x
    prism[2][1] = prism[5][1] = y
    prism[5][2] = z


class TerrainRef(PlaneRef):
    def __init__(self, model, hf, horizontal_scale, vertical_scale, origin):
        # not PlaneRef.__init__: the ground here is the heightfield; the supports need only the geoms and the cylinder table
        self.m = model
        self.geoms, self.links = model["geoms"], model["links"]
        col = model["collider"]
        self.mc_tolerance, self.n_contacts_per_pair = col["mc_tolerance"], col["n_contacts_per_pair"]
        self.ccd_eps, self.ccd_tolerance, self.ccd_iterations = col["ccd_eps"], col["ccd_tolerance"], col["ccd_iterations"]
        self.theta_to_ring = np.asarray(model["support_theta_to_ring"])
        self.hf = np.asarray(hf, np.float64) * float(vertical_scale)
        self.rows, self.cols = self.hf.shape
        self.hs = float(horizontal_scale)
        self.origin = np.asarray(origin, np.float64)
        hmin, hmax = self.hf.min(), self.hf.max()
        self.xyz_maxmin = np.array([self.rows * self.hs, self.cols * self.hs, hmax, 0.0, 0.0, hmin - 1.0])
        self.t_lo = np.array([0.0, 0.0, hmin - 1.0])
        self.t_hi = np.array([(self.rows - 1) * self.hs, (self.cols - 1) * self.hs, hmax])
        self.margin = self.tie_margin = np.inf
        self.scale = 1.0
        self.mpr_calls = 0

    def _decide(self, d):
        """A decision that can change the contact list (count, pairs, order): its distance to the threshold."""
        self.margin = min(self.margin, abs(float(d)) / (F32_UNIT * self.scale))

    def _note(self, d):
        """A choice between equivalent candidates (support ties, the cylinder table's cell edges, the portal vertex MPR replaces): it moves the
        portal and with it the contact point along a face, not the decisions above."""
        self.tie_margin = min(self.tie_margin, abs(float(d)) / (F32_UNIT * self.scale))

    # ---- contact.py ----------------------------------------------------------------------------------------------------
    def tolerance(self, i_ga):
        a = np.asarray(self.geoms[i_ga]["init_aabb"], np.float64)
        return 0.5 * self.mc_tolerance * min(np.linalg.norm(a[7] - a[0]), np.linalg.norm(self.t_hi - self.t_lo))

    # ---- supports ----------------------------------------------------------------------------------------------------------
    def support_prism(self, prism, d):
        """_func_support_prism, support_field.py:265-282."""
        self._note(d[2])
        i0 = 0 if d[2] < 0 else 3
        dots = prism[i0:i0 + 3] @ d
        best = int(np.argmax(dots))                                                # the first maximum, like the strict `>` of the loop
        for j in range(3):
            if not np.array_equal(prism[i0 + j], prism[i0 + best]):
                self._note(dots[best] - dots[j])
        return prism[i0 + best].copy()

    def _sup(self, d):
        """compute_support, mpr.py:179-202: v1 on the geom along d, v2 on the prism along -d, v = v1 - v2."""
        v1 = self.support(self._ga, d, self._pos_a, self._quat_a)
        v2 = self.support_prism(self._prism, -d)
        return v1 - v2, v1, v2

    # ---- MPR, collider/mpr.py ------------------------------------------------------------------------------------------------
    def _reach_tolerance(self, V, v, d):
        """mpr_portal_reach_tolerance, mpr.py:134-143: (dot1, threshold); the portal cannot advance when dot1 < threshold."""
        dv = v @ d
        dot1 = min(dv - V[1] @ d, dv - V[2] @ d, dv - V[3] @ d)
        return dot1, self.ccd_tolerance + self.ccd_eps * max(1.0, dot1)

    def _expand(self, V, V1, V2, v, v1, v2):
        """mpr_expand_portal, mpr.py:426-442 (the signs are noted as distances to the plane through 0, v and v0)."""
        v4v0 = np.cross(v, V[0])
        n = max(np.linalg.norm(v4v0), 1e-300)
        dot = V[1] @ v4v0
        self._note(dot / n)
        if dot > 0:
            dot = V[2] @ v4v0
            self._note(dot / n)
            i_s = 1 if dot > 0 else 3
        else:
            dot = V[3] @ v4v0
            self._note(dot / n)
            i_s = 2 if dot > 0 else 1
        V[i_s], V1[i_s], V2[i_s] = v, v1, v2

    def mpr(self, center_a, center_b):
        """func_mpr_contact_from_centers, mpr.py:686-765: None, or (normal, pos, penetration) in the heightfield's frame."""
        self.mpr_calls += 1
        eps = self.ccd_eps
        V, V1, V2 = np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 3))
        # ---- mpr_discover_portal, mpr.py:445-598 ----
        V1[0], V2[0], V[0] = center_a, center_b, center_a - center_b
        self._decide(np.abs(V[0]).max() - eps)
        if (np.abs(V[0]) < eps).all():
            V[0][0] += 10.0 * eps
        d = -unit(V[0])
        V[1], V1[1], V2[1] = self._sup(d)
        dot = V[1] @ d
        self._decide(dot - eps)
        if dot < eps:
            return None
        d = np.cross(V[0], V[1])
        self._decide(np.sqrt(d @ d) - np.sqrt(eps))
        if d @ d < eps:
            self._decide(np.abs(V[1]).max() - eps)
            pos = 0.5 * (V1[1] + V2[1])
            if (np.abs(V[1]) < eps).all():                                     # mpr_find_penetr_touch, :319-325
                return -unit(V[0]), pos, 0.0
            return -unit(V[1]), pos, float(np.linalg.norm(V[1]))               # mpr_find_penetr_segment, :328-335
        d = unit(d)
        v, v1, v2 = self._sup(d)
        dot = v @ d
        self._decide(dot - eps)
        if dot < eps:
            return None
        V[2], V1[2], V2[2] = v, v1, v2
        d = unit(np.cross(V[1] - V[0], V[2] - V[0]))
        dot = d @ V[0]
        self._decide(dot)
        if dot > 0:
            V[[1, 2]], V1[[1, 2]], V2[[1, 2]] = V[[2, 1]], V1[[2, 1]], V2[[2, 1]]
            d = -d
        trials = 0
        while True:
            v, v1, v2 = self._sup(d)
            dot = v @ d
            self._decide(dot - eps)
            if dot < eps:
                return None
            cont = False
            a = np.cross(V[1], v)
            dot = a @ V[0]
            self._decide((dot + eps) / max(np.linalg.norm(a), 1e-300))
            if dot < -eps:
                V[2], V1[2], V2[2] = v, v1, v2
                cont = True
            if not cont:
                a = np.cross(v, V[2])
                dot = a @ V[0]
                self._decide((dot + eps) / max(np.linalg.norm(a), 1e-300))
                if dot < -eps:
                    V[1], V1[1], V2[1] = v, v1, v2
                    cont = True
            if not cont:
                V[3], V1[3], V2[3] = v, v1, v2
                break
            d = unit(np.cross(V[1] - V[0], V[2] - V[0]))
            trials += 1
            if trials == 15:
                self._decide(0.0)
                return None
        # ---- mpr_refine_portal, mpr.py:232-278 ----
        while True:
            d = unit(np.cross(V[2] - V[1], V[3] - V[1]))                      # mpr_portal_dir, :112-117
            dot = V[1] @ d
            self._decide(dot + eps)
            if dot > -eps:                                                     # mpr_portal_encapsules_origin
                break
            v, v1, v2 = self._sup(d)
            dot = v @ d
            self._decide(dot + eps)
            if not dot > -eps:                                                 # mpr_portal_can_encapsule_origin
                return None
            dot1, thr = self._reach_tolerance(V, v, d)
            self._decide(dot1 - thr)
            if dot1 < thr:
                return None
            self._expand(V, V1, V2, v, v1, v2)
        # ---- mpr_find_penetration, mpr.py:338-423 ----
        it = 0
        while True:
            d = unit(np.cross(V[2] - V[1], V[3] - V[1]))
            v, v1, v2 = self._sup(d)
            dot1, thr = self._reach_tolerance(V, v, d)
            if dot1 < thr or it > self.ccd_iterations:
                if not dot1 < thr:
                    self._decide(0.0)                                            # the iteration cap decided
                # mpr_find_pos, :281-316 (no MuJoCo compatibility: the weights are taken along the portal normal)
                b = np.zeros(4)
                for i in range(1, 4):
                    i1, i2 = i % 3 + 1, (i + 1) % 3 + 1
                    b[i] = np.cross(V[i1], V[i2]) @ d
                pos = (0.5 / b.sum()) * (b @ V1 + b @ V2)
                return -d, pos, float(d @ V[1])
            self._expand(V, V1, V2, v, v1, v2)
            it += 1

    # ---- narrowphase.py:345-512 ------------------------------------------------------------------------------------------------
    def pair_setup(self, i_ga, pos, quat):
        """The pair's pose in the heightfield's frame, its bounding box and cell range: None after the early return, else
        (pos_t, quat_t, center_a, r_min, r_max, c_min, c_max, zmin)."""
        pos_t = np.asarray(pos, np.float64) - self.origin                       # the heightfield's frame: translated, not rotated
        quat_t = np.asarray(quat, np.float64)
        self.scale = max(1.0, np.abs(pos_t).max(), np.abs(pos).max())
        center_a = quat_to_R(quat_t) @ np.asarray(self.geoms[i_ga]["center"], np.float64) + pos_t
        xmm = np.zeros(6)
        for i_axis in range(3):
            for i_m in range(2):
                d = np.zeros(3)
                d[i_axis] = 1.0 if i_m == 0 else -1.0
                xmm[3 * i_m + i_axis] = self.support(i_ga, d, pos_t, quat_t)[i_axis]
        tmm = self.xyz_maxmin
        for i in range(3):
            self._decide(xmm[i + 3] - tmm[i])
            self._decide(xmm[i] - tmm[i + 3])
        if any(tmm[i] < xmm[i + 3] or tmm[i + 3] > xmm[i] for i in range(3)):
            return None
        lims = []
        for x, f in ((xmm[3] - tmm[3], np.floor), (xmm[0] - tmm[3], np.ceil), (xmm[4] - tmm[4], np.floor), (xmm[1] - tmm[4], np.ceil)):
            a = x / self.hs
            self._decide((a - np.round(a)) * self.hs)
            lims.append(int(f(a)))
        r_min, r_max, c_min, c_max = max(0, lims[0]), min(self.rows - 1, lims[1]), max(0, lims[2]), min(self.cols - 1, lims[3])
        return pos_t, quat_t, center_a, r_min, r_max, c_min, c_max, xmm[5]

    def eligible_cells(self, i_ga, pos, quat):
        """The prisms of the pair whose top reaches the geom, without the contact cap."""
        s = self.pair_setup(i_ga, pos, quat)
        if s is None:
            return 0
        _, _, _, r_min, r_max, c_min, c_max, zmin = s
        if r_max <= r_min or c_max <= c_min:
            return 0
        z = self.hf[r_min:r_max + 1, c_min:c_max + 1]
        strip = np.stack([z[:-1], z[1:]], axis=2).reshape(r_max - r_min, -1) >= zmin    # vertex (c, i) of row r at 2 (c - c_min) + i
        return int((strip[:, :-2] | strip[:, 1:-1] | strip[:, 2:]).sum())

    def pair_contacts(self, i_ga, pos, quat):
        """func_contact_mpr_terrain for geom i_ga at world pose (pos, quat): list of (normal, pos, penetration) in world coordinates."""
        s = self.pair_setup(i_ga, pos, quat)
        if s is None:
            return []
        pos_t, quat_t, center_a, r_min, r_max, c_min, c_max, zmin = s
        hs, tmm = self.hs, self.xyz_maxmin
        tol = self.tolerance(i_ga)
        self._ga, self._pos_a, self._quat_a = i_ga, pos_t, quat_t
        prism = np.zeros((6, 3))
        prism[0:3, 2] = tmm[5]
        self._prism = prism
        out = []
        for r in range(r_min, r_max):
            nvert = 0
            for c in range(c_min, c_max + 1):
                for i in range(2):
                    if len(out) >= self.n_contacts_per_pair:                    # the cap also stops the walk
                        return out
                    nvert += 1
                    add_prism_vert(prism, hs * (r + i) + tmm[3], hs * c + tmm[4], self.hf[r + i, c])
                    if nvert <= 2:
                        continue
                    top = prism[3:6, 2] - zmin
                    self._decide(top.max())
                    if not (top >= 0.0).any():
                        continue
                    res = self.mpr(center_a, prism.sum(0) / 6.0)
                    if res is None:
                        continue
                    normal, cpos, pen = res
                    cpos = cpos + self.origin
                    valid = True
                    for _, p, _ in out:
                        dist = np.linalg.norm(cpos - p)
                        self._decide(dist - tol)
                        valid = valid and not dist < tol
                    if valid:
                        out.append((normal, cpos, pen))
        return out

    def broad_pairs(self, gp, gq, robot_geoms):
        """Geoms whose AABB overlaps the heightfield's, in sweep order (ascending lower x-end)."""
        tlo, thi = self.origin + self.t_lo, self.origin + self.t_hi
        keep = []
        for i_g in robot_geoms:
            lo, hi = self.aabb(i_g, gp[i_g], gq[i_g])
            self.scale = max(1.0, np.abs(lo).max(), np.abs(hi).max())
            seps = np.concatenate([thi - lo, hi - tlo])                           # overlap iff all > 0
            for x in seps:
                self._decide(x)
            if np.all(seps > 0.0):
                keep.append((lo[0], i_g))
        keep.sort()
        return [i for _, i in keep], [x for x, _ in keep]

    def contacts(self, link_pos, link_quat, robot_geoms):
        """The heightfield contacts of one collision pass: [(geom_a, 0, normal, pos, penetration)] in list order (they follow the convex-convex
        contacts).  `robot_geoms`: the geoms that the model pairs with the ground."""
        self.margin = self.tie_margin = np.inf
        gp, gq = self.geom_poses(link_pos, link_quat)
        order, xmin = self.broad_pairs(gp, gq, robot_geoms)
        out, xs = [], []
        for i_g, x in zip(order, xmin):
            cs = self.pair_contacts(i_g, gp[i_g], gq[i_g])
            if cs:
                xs.append(x)
            out += [(i_g, 0, n, p, d) for n, p, d in cs]
        for a, b in zip(xs[:-1], xs[1:]):                                         # the order of the pairs that produce contacts
            self.scale = max(1.0, abs(a), abs(b))
            self._decide(b - a)
        return out

    def eligible_total(self, link_pos, link_quat, robot_geoms):
        """Prism descriptors of one collision pass before any cap: the eligible prisms of every pair."""
        gp, gq = self.geom_poses(link_pos, link_quat)
        order, _ = self.broad_pairs(gp, gq, robot_geoms)
        return sum(self.eligible_cells(i_g, gp[i_g], gq[i_g]) for i_g in order)
