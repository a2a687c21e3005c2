"""The case table of the mirror-symmetry tests (tests/test_ppo_sym_gpu.py, tests/test_ppo_sym_ref.py, tests/test_mirror_tables.py): the mirrors as
literal tables, the networks, row counts and inputs.  The original rows come from tests/ppo_cases.py (every branch decision of the law has a margin);
the mirrored rows' ratios and values fall where the networks put them, so a case asserts its own promises on them: margins to every branch point,
rows whose ratio is inside the clip range on the original and outside it on the mirror (and only there), value-clip ties (|v - target_values| inside
the clip range: both arms of the max are the same function) on both halves.  A case's float64 and float32 evaluations are computed once and shared."""
import functools

import torch

import ppo_cases as PC
import ppo_ref as R
import ppo_sym_ref as SR


def _table(src, signs):
    assert len(src) == len(signs)
    return torch.tensor(src, dtype=torch.int32), torch.tensor([1.0 if c == "+" else -1.0 for c in signs], dtype=torch.float32)


# Go2Env's layouts written out entry by entry (include/go2sim.h's observation order; joints FR, FL, RR, RL x hip, thigh, calf):
#   obs     angular velocity 3 | gravity 3 | commands 3 | dof pos 12 | dof vel 12 | actions 12 (+ 4 per-leg stiffness)
#   critic  obs | base lin vel 3 | friction | kp 12 | kd 12 | motor strength 12 | mass shift | com shift 3 | leg mass shifts 4 | gravity offset 3 |
#           push force 3 | delay (| terrain row | 11 x 7 height scan, index ix * 7 + iy)
_LITERAL = {
    "walk": {
        "policy": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41, 46, 45, 48, 47],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-++++++"),
        "critic": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41, 46, 45, 48, 47, 49, 50, 51, 52, 56, 57, 58, 53, 54, 55, 62, 63, 64, 59, 60,
            61, 68, 69, 70, 65, 66, 67, 74, 75, 76, 71, 72, 73, 80, 81, 82, 77, 78, 79, 86, 87, 88, 83, 84, 85, 89, 90, 91, 92,
            94, 93, 96, 95, 97, 98, 99, 100, 101, 102, 103],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-+++++++-++++++++++++++++++++++++++++++++++++++++-++++++-++-++"),
        "actions": ([3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8, 13, 12, 15, 14],
            "-++-++-++-++++++"),
    },
    "pls_off": {
        "policy": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-++"),
        "critic": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41, 45, 46, 47, 48, 52, 53, 54, 49, 50, 51, 58, 59, 60, 55, 56, 57, 64, 65, 66,
            61, 62, 63, 70, 71, 72, 67, 68, 69, 76, 77, 78, 73, 74, 75, 82, 83, 84, 79, 80, 81, 85, 86, 87, 88, 90, 89, 92, 91,
            93, 94, 95, 96, 97, 98, 99],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-+++-++++++++++++++++++++++++++++++++++++++++-++++++-++-++"),
        "actions": ([3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8],
            "-++-++-++-++"),
    },
    "stairs": {
        "policy": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41, 46, 45, 48, 47],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-++++++"),
        "critic": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41, 46, 45, 48, 47, 49, 50, 51, 52, 56, 57, 58, 53, 54, 55, 62, 63, 64, 59, 60,
            61, 68, 69, 70, 65, 66, 67, 74, 75, 76, 71, 72, 73, 80, 81, 82, 77, 78, 79, 86, 87, 88, 83, 84, 85, 89, 90, 91, 92,
            94, 93, 96, 95, 97, 98, 99, 100, 101, 102, 103, 104, 111, 110, 109, 108, 107, 106, 105, 118, 117, 116, 115, 114, 113,
            112, 125, 124, 123, 122, 121, 120, 119, 132, 131, 130, 129, 128, 127, 126, 139, 138, 137, 136, 135, 134, 133, 146,
            145, 144, 143, 142, 141, 140, 153, 152, 151, 150, 149, 148, 147, 160, 159, 158, 157, 156, 155, 154, 167, 166, 165,
            164, 163, 162, 161, 174, 173, 172, 171, 170, 169, 168, 181, 180, 179, 178, 177, 176, 175],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-+++++++-++++++++++++++++++++++++++++++++++++++++-++++++-++-"
            "++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++"),
        "actions": ([3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8, 13, 12, 15, 14],
            "-++-++-++-++++++"),
    },
    "base": {
        "policy": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-++"),
        "critic": ([0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 24, 25, 26, 21, 22, 23, 30, 31, 32, 27, 28, 29, 36, 37,
            38, 33, 34, 35, 42, 43, 44, 39, 40, 41],
            "-+-+-++---++-++-++-++-++-++-++-++-++-++-++-++"),
        "actions": ([3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8],
            "-++-++-++-++"),
    },
}
ENV_TABLES = {name: {k: _table(*v) for k, v in t.items()} for name, t in _LITERAL.items()}

# the small pair: fixed points, swaps only (no longer cycle), mixed signs
SMALL_NETS = ([7, 16, 3], [9, 16, 1])
SMALL_TABLES = {
    "policy": _table([1, 0, 2, 4, 3, 5, 6], "---++-+"),
    "critic": _table([2, 1, 0, 3, 4, 8, 6, 7, 5], "+-+-+-++-"),
    "actions": _table([2, 1, 0], "-+-"),
}
WALK_NETS = ([49, 512, 256, 128, 16], [104, 512, 256, 128, 1])
FLAGS = {"augment": (True, False, 0.0), "mirror": (False, True, 0.5), "both": (True, True, 0.5)}          # (augmentation, mirror loss, coefficient)
# (name, rows): 2 n = 34 ragged tiles; 600: both halves share the first row chunk, the mirrored half straddles its end; 1024: the mirrored half is
# exactly the second chunk; the walk shapes with Go2Env's real tables
SHAPES = [("small", 17), ("small", 300), ("small", 512), ("walk", 37)]
MARGIN = 1e-4                                               # of a ratio or a value of order 1: a hundred float32 roundings of the forward pass


class Case:
    def __init__(self, shape, n_rows, seed):
        self.shape, self.n = shape, n_rows
        self.adims, self.cdims = SMALL_NETS if shape == "small" else WALK_NETS
        self.tables = SMALL_TABLES if shape == "small" else ENV_TABLES["walk"]
        total = n_rows + 3
        g = torch.Generator().manual_seed(seed)
        self.state = PC.init_state(self.adims, self.cdims, g)
        perm = torch.randperm(total, generator=g)
        self.idx = perm[:n_rows].to(torch.int32)
        ro = PC.make_rollout(self.adims, self.cdims, self.state, n_rows, "keep", seed + 1)
        self.rollout = {k: torch.full((total,) + tuple(x.shape[1:]), float("nan")) for k, x in ro.items()}
        for k, x in ro.items():
            self.rollout[k][self.idx.long()] = x
        self.check_mirrored_rows()
        self._ref = {}

    def rows(self, dtype):
        return R.rows_of(self.rollout, self.idx.long(), dtype)

    def check_mirrored_rows(self, hp=R.HP):
        """what the module docstring promises of the mirrored half"""
        clip, n = hp["clip_param"], self.n
        m64 = R.make_model(self.adims, self.cdims, self.state, torch.float64)
        mb = self.rows(torch.float64)
        with torch.no_grad():
            _, t = SR.loss_terms(m64, mb, self.tables, True, True, 0.5, hp)
            _, t2 = R.head_terms(t["mu2"], m64.std, t["v2"], SR.doubled(mb, self.tables), hp)
        ratio, v = t2["ratio"], t["v2"]
        assert bool((((ratio - (1 - clip)).abs() > MARGIN) & ((ratio - (1 + clip)).abs() > MARGIN)).all())
        inside = (ratio >= 1 - clip) & (ratio <= 1 + clip)
        assert int((inside[:n] & ~inside[n:]).sum()) >= 1, "no row leaves the clip range on the mirrored side only"
        tv, ret = torch.cat([mb["target_values"]] * 2), torch.cat([mb["returns"]] * 2)
        d = (v - tv).abs()
        assert bool(((d - clip).abs() > MARGIN).all())
        assert int((d[:n] < clip).sum()) >= 1 and int((d[n:] < clip).sum()) >= 1 and int((d[n:] > clip).sum()) >= 1, "value-clip ties on both halves"
        vc = tv + (v - tv).clamp(-clip, clip)
        assert bool(((ret - (v + vc) / 2).abs()[d > clip] > MARGIN).all())
        kl, dkl = float(t["kl_mean"]), hp["desired_kl"]
        assert 1.2 * dkl / 2 < kl < 0.8 * 2 * dkl, kl

    def ref(self, flags):
        """{"f64" | "f32": (grads, scalars)} under FLAGS[flags]"""
        if flags not in self._ref:
            aug, mloss, coeff = FLAGS[flags]
            self._ref[flags] = {name: SR.minibatch_grad(R.make_model(self.adims, self.cdims, self.state, dt), self.rows(dt), self.tables, aug, mloss, coeff)
                                for name, dt in (("f64", torch.float64), ("f32", torch.float32))}
        return self._ref[flags]


@functools.lru_cache(maxsize=None)
def get_case(shape, n_rows):
    return Case(shape, n_rows, seed=SEEDS[(shape, n_rows)])


SEEDS = {("small", 17): 9100, ("small", 300): 9200, ("small", 512): 9300, ("walk", 37): 9400, ("small", 37): 9500}


@functools.lru_cache(maxsize=None)
def get_update_case(flags="both"):
    """2 epochs x 2 mini-batches of 37 rows on the small pair, float64 and float32 whole updates"""
    rows, epochs, n_mb = 74, 2, 2
    adims, cdims = SMALL_NETS
    g = torch.Generator().manual_seed(9600)
    state = PC.init_state(adims, cdims, g)
    ro = PC.make_rollout(adims, cdims, state, rows, "keep", 9601)
    perm = torch.randperm(rows, generator=g).to(torch.int32)
    aug, mloss, coeff = FLAGS[flags]
    out = dict(adims=adims, cdims=cdims, state=state, rollout=ro, perm=perm, rows=rows, epochs=epochs, n_mb=n_mb, tables=SMALL_TABLES)
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = R.make_model(adims, cdims, state, dt)
        means, lr = SR.update(m, ro, perm, epochs, n_mb, SMALL_TABLES, aug, mloss, coeff)
        out[prec] = dict(params={k: p.detach().clone() for k, p in R.ordered_params(m)}, means=means, lr=lr)
    return out
