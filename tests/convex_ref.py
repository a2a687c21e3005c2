"""Float64 geometry of convex pairs and a numpy float64 restatement of the convex-convex pair loop, independent of the library's code.

(a) Geometry.  A geom is a convex body with a support height h_X(d) = max of x . d over X.  For two posed geoms and a unit direction d (from b
    towards a) the overlap width is w(d) = h_b(d) + h_a(-d); the penetration depth is min_d w(d) and the geoms overlap iff it is positive.
      * `h` / `w` evaluate tests/plane_ref.py's support functions (the cylinder through the model's 180 x 180 support table with its 32-gon rim: the
        shape the collider sees);
      * `heights` / `widths` are the same for many directions at once, from the vertices of that shape (box: 8 corners, cylinder: the 2 x 32 rim
        vertices, sphere: centre and radius);
      * `min_width` searches the minimum: a few thousand Fibonacci directions, the face normals and edge-edge cross products of the two polytopes
        (where the minimum of a polytope pair lies), the directions from a polytope's vertices and edges to a sphere's centre, then a shrinking
        local refinement from the best starts.  The result is an UPPER BOUND of the true depth (`upper_bound=True` in what it returns);
      * `contains` tests p . d <= h(d) + tol over sampled directions plus the geom's own face / axis directions;
      * `slab_closed_form`: a geom against the ground slab: the depth of its support point along the slab's inward normal, that point, and the gap
        to the second-best distinct support candidate (the tie margin).
(b) Pair loop: func_convex_convex_contact (narrowphase.py:514-961, the non-plane branch, CCD_ALGORITHM_CODE.MPR): MPR from the cached normal
    (mpr.py:601-819: guess_geoms_center with its offset branch, then tests/terrain_ref.py's MPR over the two geoms' supports), the retry without the
    guess when the first detection misses, prefer_gjk = penetration > tolerance and (no guess or mc_tolerance * pen >= mpr_to_gjk_overlap_ratio *
    tolerance), the four perturbed detections (qrot on a, inv(qrot) on b, about the first contact), their position / normal / penetration correction,
    the de-duplication against the pair's earlier contacts, `penetration > -tolerance`, and the write-back of the normal cache.  Where the loop takes
    the GJK / EPA branch this reference does NOT restate EPA: it answers with the geometric truth of (a) -- the minimum-width direction and depth, the
    closed form on the slab, the contact on the mid-plane between the two support points -- and marks the contact `fallback`.
    A pair that a coarse direction search shows to be more than 1 mm apart is not run through MPR: every detection misses there.
    Broad phase for the box ground: the pairs of the model's pair table whose world AABBs overlap (`overlapping_pairs`); their order in the contact
    list, the sweep's, is restated next to the test's margin in tests/convex_cases.py (PipelineRef.ordered).
    Every keep / drop / branch decision records its distance to the threshold: the MPR-internal ones through `_decide` / `_note` (`margin`,
    `tie_margin`: terrain_ref.py), the loop's own in metres (`loop_margin`): penetration against the tolerance and against the GJK switch, the
    centre-offset test, de-duplication distances, `> -tolerance`, the orthogonals' axis choice, the AABB overlap of the pairs that produce a contact,
    and for a fallback answer the width's sign, a second minimum of the width in another direction and the uniqueness of the witness point."""
import numpy as np

from plane_ref import GEOM_BOX, GEOM_CYLINDER, GEOM_SPHERE, inv_quat, quat_to_R, rotate_frame, rotvec_to_quat
from terrain_ref import TerrainRef, unit


def fibonacci(n):
    i = np.arange(n) + 0.5
    ph, th = np.arccos(1.0 - 2.0 * i / n), np.pi * (1.0 + 5.0 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)], axis=1)


SPHERE_DIRS = fibonacci(4000)
AXES = np.concatenate([np.eye(3), -np.eye(3)])


class ConvexRef(TerrainRef):
    def __init__(self, model):
        # not TerrainRef.__init__: there is no heightfield; its MPR needs the collider constants and the two supports (_sup below)
        self.m = model
        self.geoms, self.links = model["geoms"], model["links"]
        col = model["collider"]
        self.mc_tolerance, self.mc_perturbation, self.n_contacts_per_pair = col["mc_tolerance"], col["mc_perturbation"], col["n_contacts_per_pair"]
        self.mpr_to_gjk = col["mpr_to_gjk_overlap_ratio"]
        self.ccd_eps, self.ccd_tolerance, self.ccd_iterations = col["ccd_eps"], col["ccd_tolerance"], col["ccd_iterations"]
        self.eps = model["eps"]
        self.theta_to_ring = np.asarray(model["support_theta_to_ring"])
        ng = len(self.geoms)
        self.pair_idx = np.asarray(model["collision_pair_idx"]).reshape(ng, ng)
        self.margin = self.tie_margin = self.loop_margin = np.inf
        self.scale = 1.0
        self.mpr_calls = 0
        self._shape = {}

    def _loop(self, d):
        """A decision of the pair loop itself, in metres (or in the units of the compared quantity)."""
        self.loop_margin = min(self.loop_margin, abs(float(d)))

    # ---- (a) geometry ------------------------------------------------------------------------------------------------------
    def shape(self, i_g):
        """(local vertices, radius, local face normals, local edge directions, edges as vertex index pairs) of the shape the collider sees."""
        if i_g not in self._shape:
            g = self.geoms[i_g]
            if g["type"] == GEOM_SPHERE:
                s = (np.zeros((1, 3)), float(g["data"][0]), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2), int))
            elif g["type"] == GEOM_BOX:
                hs = 0.5 * np.asarray(g["data"][:3], np.float64)
                sg = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
                e = [(i, j) for i in range(8) for j in range(i + 1, 8) if np.abs(sg[i] - sg[j]).sum() == 2.0]
                s = (sg * hs, 0.0, np.eye(3), np.eye(3), np.array(e))
            elif g["type"] == GEOM_CYLINDER:
                rim, half = np.asarray(g["rim"], np.float64), 0.5 * g["data"][1]
                n = len(rim)
                v = np.concatenate([np.c_[rim, np.full(n, half)], np.c_[rim, np.full(n, -half)]])
                nxt = np.roll(rim, -1, axis=0)
                ed = np.c_[nxt - rim, np.zeros(n)]
                side = np.c_[ed[:, 1], -ed[:, 0], np.zeros(n)]
                e = [(i, (i + 1) % n) for i in range(n)] + [(n + i, n + (i + 1) % n) for i in range(n)] + [(i, n + i) for i in range(n)]
                s = (v, 0.0, np.concatenate([[[0.0, 0.0, 1.0]], side / np.linalg.norm(side, axis=1)[:, None]]),
                     np.concatenate([[[0.0, 0.0, 1.0]], ed / np.linalg.norm(ed, axis=1)[:, None]]), np.array(e))
            else:
                raise ValueError("no shape for geom type %d" % g["type"])
            self._shape[i_g] = s
        return self._shape[i_g]

    def world_verts(self, i_g, pos, quat):
        return self.shape(i_g)[0] @ quat_to_R(quat).T + np.asarray(pos, np.float64)

    def h(self, i_g, d, pos, quat):
        """Support height along the unit direction d, through PlaneRef.support."""
        d = np.asarray(d, np.float64)
        return float(self.support(i_g, d, np.asarray(pos, np.float64), np.asarray(quat, np.float64)) @ d)

    def w(self, i_ga, i_gb, d, pa, qa, pb, qb):
        d = np.asarray(d, np.float64)
        return self.h(i_gb, d, pb, qb) + self.h(i_ga, -d, pa, qa)

    def heights(self, i_g, D, pos, quat):
        return (D @ self.world_verts(i_g, pos, quat).T).max(axis=1) + self.shape(i_g)[1]

    def widths(self, i_ga, i_gb, D, pa, qa, pb, qb):
        return self.heights(i_gb, D, pb, qb) + self.heights(i_ga, -D, pa, qa)

    def feature_dirs(self, i_ga, i_gb, pa, qa, pb, qb):
        """Directions at which the minimum width of the pair can lie besides a smooth interior minimum: face normals, edge x edge, and, against a
        sphere, the directions from the other geom's vertices and edges (closest points) to the sphere's centre."""
        Ra, Rb = quat_to_R(qa), quat_to_R(qb)
        sa, sb = self.shape(i_ga), self.shape(i_gb)
        out = [sa[2] @ Ra.T, sb[2] @ Rb.T]
        ea, eb = sa[3] @ Ra.T, sb[3] @ Rb.T
        if len(ea) and len(eb):
            out.append(np.cross(ea[:, None, :], eb[None, :, :]).reshape(-1, 3))
        for (i_s, ps), (i_p, pp, qp) in (((i_ga, pa), (i_gb, pb, qb)), ((i_gb, pb), (i_ga, pa, qa))):
            if self.geoms[i_s]["type"] == GEOM_SPHERE and self.geoms[i_p]["type"] != GEOM_SPHERE:
                v = self.world_verts(i_p, pp, qp)
                e = self.shape(i_p)[4]
                p0, p1 = v[e[:, 0]], v[e[:, 1]]
                t = np.clip(((ps - p0) * (p1 - p0)).sum(1) / ((p1 - p0) ** 2).sum(1), 0.0, 1.0)
                out += [ps - v, ps - (p0 + t[:, None] * (p1 - p0))]
        if self.geoms[i_ga]["type"] == GEOM_SPHERE and self.geoms[i_gb]["type"] == GEOM_SPHERE:
            out.append((np.asarray(pa) - np.asarray(pb))[None])
        D = np.concatenate(out)
        nrm = np.linalg.norm(D, axis=1)
        D = D[nrm > 1e-12] / nrm[nrm > 1e-12, None]
        return np.concatenate([D, -D])

    def min_width(self, i_ga, i_gb, pa, qa, pb, qb, refine=True, starts=3, rounds=40, seed=0):
        """dict(w, d, upper_bound=True): the smallest overlap width found and its direction (from b towards a)."""
        pa, qa, pb, qb = (np.asarray(x, np.float64) for x in (pa, qa, pb, qb))
        D = np.concatenate([SPHERE_DIRS if refine else SPHERE_DIRS[::4], self.feature_dirs(i_ga, i_gb, pa, qa, pb, qb)])
        Va, Vb, rr = self.world_verts(i_ga, pa, qa).T, self.world_verts(i_gb, pb, qb).T, self.shape(i_ga)[1] + self.shape(i_gb)[1]
        widths = lambda X: (X @ Vb).max(axis=1) + (-X @ Va).max(axis=1) + rr          # self.widths on the posed vertices
        ws = widths(D)
        order = np.argsort(ws)
        best_w, best_d = ws[order[0]], D[order[0]]
        second = np.inf                                                              # the best local minimum in another direction (> 0.1 rad away)
        if refine:
            rng = np.random.default_rng(seed)
            found = []
            picked = []
            for k in order:                                                         # distinct starts: more than 0.1 rad apart
                if all(D[k] @ D[j] < np.cos(0.1) for j in picked):
                    picked.append(k)
                if len(picked) == starts:
                    break
            for k in picked:
                d0, w0, s = D[k], ws[k], 0.05
                for _ in range(rounds):
                    C = d0 + s * rng.standard_normal((48, 3))
                    C /= np.linalg.norm(C, axis=1)[:, None]
                    wc = widths(C)
                    j = int(np.argmin(wc))
                    if wc[j] < w0:
                        d0, w0 = C[j], wc[j]
                    else:
                        s *= 0.5
                found.append((w0, d0))
            found.sort(key=lambda f: f[0])
            best_w, best_d = found[0]
            others = [f[0] for f in found[1:] if f[1] @ best_d < np.cos(0.1)]
            if others:
                second = min(others)
        return dict(w=float(best_w), d=best_d, upper_bound=True, second=float(second))

    def own_dirs(self, i_g, quat):
        F = self.shape(i_g)[2] @ quat_to_R(quat).T
        return np.concatenate([F, -F]) if len(F) else np.zeros((0, 3))

    def outside(self, i_g, p, pos, quat):
        """How far p lies outside the geom: max over the sampled and the geom's own directions of p . d - h(d) (negative inside)."""
        D = np.concatenate([SPHERE_DIRS, AXES, self.own_dirs(i_g, quat)])
        return float((D @ np.asarray(p, np.float64) - self.heights(i_g, D, pos, quat)).max())

    def contains(self, i_g, p, pos, quat, tol=0.0):
        return self.outside(i_g, p, pos, quat) <= tol

    def slab_closed_form(self, i_g, pos, quat, slab_pos, slab_quat, i_slab=0):
        """dict(depth, point, tie): the geom's support point along the slab's inward normal (the slab's top face is its local +z face), its depth
        below that face, and the gap in depth to the next distinct support candidate (inf for a sphere)."""
        pos, quat = np.asarray(pos, np.float64), np.asarray(quat, np.float64)
        up = quat_to_R(slab_quat)[:, 2]
        top = np.asarray(slab_pos, np.float64) @ up + 0.5 * self.geoms[i_slab]["data"][2]
        p = self.support(i_g, -up, pos, quat)
        depth = top - p @ up
        tie = np.inf
        if self.geoms[i_g]["type"] != GEOM_SPHERE:
            v = self.world_verts(i_g, pos, quat)
            z = np.sort(v @ up)
            tie = float(z[1] - z[0])
            p = v[int(np.argmin(v @ up))]
            depth = top - p @ up
        return dict(depth=float(depth), point=p, tie=tie)

    # ---- (b) contact.py ----------------------------------------------------------------------------------------------------------
    def diag(self, i_g):
        a = np.asarray(self.geoms[i_g]["init_aabb"], np.float64)
        return np.linalg.norm(a[7] - a[0])

    def tolerance(self, i_ga, i_gb):
        """func_compute_tolerance, contact.py:264-283."""
        return 0.5 * self.mc_tolerance * min(self.diag(i_ga), self.diag(i_gb))

    def orthogonals(self, i_ga, i_gb, normal, link_quat):
        """func_contact_orthogonals, contact.py:286-345: the geom with the smaller prod(init_aabb[7]) gives the inertial frame."""
        va, vb = (float(np.prod(np.asarray(self.geoms[i]["init_aabb"], np.float64)[7])) for i in (i_ga, i_gb))
        if va != vb:                                                                # equal boxes (two calves): both precisions take b
            self._loop((va - vb) / max(va, vb))
        i_g = i_ga if va < vb else i_gb
        rot = quat_to_R(self.inertial_quat(link_quat, self.geoms[i_g]["link"]))
        ang = np.abs(rot.T @ normal)
        order = np.argsort(-ang, kind="stable")
        self._loop(ang[order[0]] - ang[order[1]])
        a0 = rot[:, (int(order[0]) + 1) % 3]
        a0 = unit(a0 - normal.dot(a0) * normal)
        return a0, np.cross(normal, a0)

    # ---- mpr.py ----------------------------------------------------------------------------------------------------------------------
    def _sup(self, d):
        """compute_support, mpr.py:179-202, over the two geoms' supports."""
        v1 = self.support(self._ga, d, self._pos_a, self._quat_a)
        v2 = self.support(self._gb, -d, self._pos_b, self._quat_b)
        return v1 - v2, v1, v2

    def guess_centers(self, i_ga, i_gb, pa, qa, pb, qb, normal_ws):
        """guess_geoms_center, mpr.py:601-683."""
        Ra, Rb = quat_to_R(qa), quat_to_R(qb)
        ca = Ra @ np.asarray(self.geoms[i_ga]["center"], np.float64) + pa
        cb = Rb @ np.asarray(self.geoms[i_gb]["center"], np.float64) + pb
        if (np.abs(normal_ws) > self.ccd_eps).any():
            A, B = (np.asarray(self.geoms[i]["init_aabb"], np.float64) for i in (i_ga, i_gb))
            ca, cb = Ra @ (0.5 * (A[7] + A[0])) + pa, Rb @ (0.5 * (B[7] + B[0])) + pb
            delta = ca - cb
            s = np.linalg.norm(np.cross(normal_ws, unit(delta)))
            self._loop(s - 0.01)
            if s > 0.01:
                offset = delta.dot(normal_ws) * normal_ws - delta
                on = np.linalg.norm(offset)
                if on > self.eps:
                    do = offset / on
                    la, lb = (A[7] - A[0]) @ np.abs(Ra.T @ do), (B[7] - B[0]) @ np.abs(Rb.T @ do)
                    ratio = min(on / (la + lb), 0.5)
                    ca, cb = ca + do * la * ratio, cb - do * lb * ratio
        return ca, cb

    def mpr_contact(self, i_ga, i_gb, pa, qa, pb, qb, normal_ws):
        """func_mpr_contact, mpr.py:768-819: None, or (normal, pos, penetration)."""
        self._ga, self._pos_a, self._quat_a, self._gb, self._pos_b, self._quat_b = i_ga, pa, qa, i_gb, pb, qb
        self.scale = max(1.0, np.abs(self.world_verts(i_ga, pa, qa)).max(), np.abs(self.world_verts(i_gb, pb, qb)).max())
        ca, cb = self.guess_centers(i_ga, i_gb, pa, qa, pb, qb, normal_ws)
        return self.mpr(ca, cb)

    # ---- the GJK / EPA branch: the geometric truth, not EPA ------------------------------------------------------------------------
    def support_face(self, i_g, d, pos, quat):
        """(points, gap): the points of the geom that tie for the support along d (within 1e-9 m; a sphere has one) and how far the next
        candidate lies behind them."""
        if self.geoms[i_g]["type"] == GEOM_SPHERE:
            return (np.asarray(pos, np.float64) + self.geoms[i_g]["data"][0] * d)[None], np.inf
        v = self.world_verts(i_g, pos, quat)
        hs = v @ d
        tied = hs >= hs.max() - 1e-9
        return v[tied], float(hs.max() - hs[~tied].max())

    def witness(self, i_ga, i_gb, n, w, pa, qa, pb, qb):
        """The contact point of the minimum-width direction n (width w): the midpoint of a on A's support face along -n and b = a + w n on B's
        along n, where that pair is unique: a vertex (or a sphere) against anything, or two crossing edges.  Returns (pos, margin): margin is the
        gap to the next support candidate, 0 where the faces overlap in more than a point (parallel features)."""
        FA, gap_a = self.support_face(i_ga, -n, pa, qa)
        FB, gap_b = self.support_face(i_gb, n, pb, qb)
        if len(FA) == 1 and (len(FB) > 1 or gap_a >= gap_b):
            return FA[0] + 0.5 * w * n, gap_a
        if len(FB) == 1:
            return FB[0] - 0.5 * w * n, gap_b
        if len(FA) == 2 and len(FB) == 2:                                           # edge against edge: where they cross, seen along n
            e1 = unit(np.cross(n, FA[1] - FA[0]))
            e2 = np.cross(n, e1)
            P = np.stack([e1, e2])
            M = np.stack([P @ (FA[1] - FA[0]), -(P @ (FB[1] - FB[0]))], axis=1)
            if abs(np.linalg.det(M)) > 1e-12:
                s_, t_ = np.linalg.solve(M, P @ (FB[0] - FA[0]))
                inside = min(s_, 1.0 - s_, t_, 1.0 - t_)
                if inside > 0.0:
                    a = FA[0] + s_ * (FA[1] - FA[0])
                    return a + 0.5 * w * n, min(gap_a, gap_b, inside * min(np.linalg.norm(FA[1] - FA[0]), np.linalg.norm(FB[1] - FB[0])))
        return 0.5 * (FA.mean(0) + FB.mean(0)), 0.0

    def truth_contact(self, i_ga, i_gb, pa, qa, pb, qb):
        """None when the geoms are apart, else (normal, pos, penetration) of the minimum-width direction, pos from `witness`.  Against the ground
        slab (a 100 m half-width box) the closed form.  The width's sign and the uniqueness of the contact point go into `loop_margin`."""
        big = [self.diag(i) > 50.0 for i in (i_ga, i_gb)]
        if big[0] or big[1]:
            i_s, ps, qs, i_r, pr, qr = (i_ga, pa, qa, i_gb, pb, qb) if big[0] else (i_gb, pb, qb, i_ga, pa, qa)
            c = self.slab_closed_form(i_r, pr, qr, ps, qs, i_slab=i_s)
            up = quat_to_R(qs)[:, 2]
            n = -up if big[0] else up                                               # from b to a
            self._loop(c["depth"])
            if not c["depth"] > 0.0:
                return None
            self._loop(10.0 * c["tie"])                                             # 1e-5 m between candidates is as good as 1e-4 elsewhere
            return n, c["point"] + 0.5 * c["depth"] * up, c["depth"]
        r = self.min_width(i_ga, i_gb, pa, qa, pb, qb)
        self._loop(r["w"])
        if not r["w"] > 0.0:
            return None
        self._loop(r["second"] - r["w"])                                            # another direction nearly as shallow: either normal is right
        pos, margin = self.witness(i_ga, i_gb, r["d"], r["w"], pa, qa, pb, qb)
        self._loop(10.0 * margin)
        return r["d"], pos, r["w"]

    # ---- narrowphase.py:514-961 ---------------------------------------------------------------------------------------------------------
    def pair_contacts(self, i_ga, i_gb, gp, gq, link_quat, cache):
        """func_convex_convex_contact for (a, b) with type_a <= type_b.  `cache`: the pair's cached normal.  Returns (contacts, new cache, info):
        contacts = [dict(normal, pos, pen, fallback, det: the detection 0..4)], info = dict(n_fallback detections, retried)."""
        multi = self.geoms[i_ga]["type"] != GEOM_SPHERE and self.geoms[i_gb]["type"] != GEOM_SPHERE
        tol = self.tolerance(i_ga, i_gb)
        pa0, qa0, pb0, qb0 = gp[i_ga], gq[i_ga], gp[i_gb], gq[i_gb]
        cache = np.asarray(cache, np.float64).copy()
        out, info = [], dict(n_fallback=0, retried=False)
        gap = -self.min_width(i_ga, i_gb, pa0, qa0, pb0, qb0, refine=False)["w"]
        if gap > 1e-3:                  # a separating direction with a millimetre to spare: every detection misses, with or without a guess
            return out, np.zeros(3), info
        col0 = None
        ax0 = ax1 = None
        for i_det in range(5):
            if i_det > 0 and not (multi and col0 is not None):
                break
            pa, qa, pb, qb = pa0, qa0, pb0, qb0
            qrot = None
            if i_det > 0:
                axis = (2 * (i_det % 2) - 1) * ax0 + (1 - 2 * ((i_det // 2) % 2)) * ax1
                qrot = rotvec_to_quat(self.mc_perturbation * axis)
                pa, qa = rotate_frame(pa0, qa0, col0[1], qrot)
                pb, qb = rotate_frame(pb0, qb0, col0[1], inv_quat(qrot))
            normal_ws = cache.copy()
            guess = bool((np.abs(normal_ws) > self.eps).any())
            res = self.mpr_contact(i_ga, i_gb, pa, qa, pb, qb, normal_ws)
            if i_det == 0 and res is None and guess:
                normal_ws, guess = np.zeros(3), False
                info["retried"] = True
                res = self.mpr_contact(i_ga, i_gb, pa, qa, pb, qb, normal_ws)
            fallback = False
            pen = res[2] if res is not None else 0.0
            self._loop(pen - tol)
            if pen > tol:
                if guess:
                    self._loop(pen - self.mpr_to_gjk * tol / self.mc_tolerance)
                fallback = (not guess) or self.mc_tolerance * pen >= self.mpr_to_gjk * tol
            if fallback:
                info["n_fallback"] += 1
                res = self.truth_contact(i_ga, i_gb, pa, qa, pb, qb)
            if i_det == 0:
                if res is None:
                    return out, np.zeros(3), info
                col0 = res
                out.append(dict(normal=res[0], pos=res[1], pen=res[2], fallback=fallback, det=0))
                cache = np.asarray(res[0], np.float64).copy()
                if multi:
                    ax0, ax1 = self.orthogonals(i_ga, i_gb, res[0], link_quat)
                continue
            if res is None:
                continue
            normal, cpos, pen = res
            Rq = quat_to_R(qrot)
            cpa = Rq.T @ ((cpos - 0.5 * pen * normal) - col0[1]) + col0[1]
            cpb = Rq @ ((cpos + 0.5 * pen * normal) - col0[1]) + col0[1]
            cpos = 0.5 * (cpa + cpb)
            tw = np.cross(normal, col0[0])
            normal = normal + np.cross(np.clip(tw, -self.mc_perturbation, self.mc_perturbation), normal)
            pen = float(normal @ (cpb - cpa))
            repeated = False
            for prev in out:
                dist = np.linalg.norm(cpos - prev["pos"])
                if not repeated:
                    self._loop(dist - tol)
                repeated = repeated or dist < tol
            if repeated:
                continue
            self._loop(pen + tol)
            if pen > -tol:
                out.append(dict(normal=normal, pos=cpos, pen=max(pen, 0.0), fallback=fallback, det=i_det))
        return out, cache, info

    # ---- broad phase ------------------------------------------------------------------------------------------------------------------------
    def overlapping_pairs(self, gp, gq):
        """The pairs of the model's pair table whose world AABBs (init-AABB corners moved to the world) overlap: {(i, j): the smallest overlap},
        i < j.  Geoms whose boxes are apart are apart; the overlap of a pair goes into `loop_margin` only if the pair produces a contact."""
        ng = len(self.geoms)
        box = [self.aabb(i, gp[i], gq[i]) for i in range(ng)]
        keep = {}
        for i in range(ng):
            for j in range(i + 1, ng):
                if self.pair_idx[i, j] < 0:
                    continue
                seps = np.concatenate([box[j][1] - box[i][0], box[i][1] - box[j][0]])
                if np.all(seps > 0.0):
                    keep[(i, j)] = float(seps.min())
        return keep

    def contacts(self, link_pos, link_quat, caches):
        """One collision pass on the box ground.  caches: {(i, j): normal} (missing: zero).  Returns {(i_ga, i_gb): (contacts, new cache, info)} with
        (i_ga, i_gb) ordered by type as the narrow phase orders them (the lower index first among equal types)."""
        self.margin = self.tie_margin = self.loop_margin = np.inf
        gp, gq = self.geom_poses(link_pos, link_quat)
        out = {}
        for (i, j), overlap in sorted(self.overlapping_pairs(gp, gq).items()):
            a, b = (j, i) if self.geoms[i]["type"] > self.geoms[j]["type"] else (i, j)
            out[(a, b)] = self.pair_contacts(a, b, gp, gq, link_quat, caches.get((i, j), np.zeros(3)))
            if out[(a, b)][0]:
                self._loop(overlap)
        return out
