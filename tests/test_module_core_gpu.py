"""The four policy modules under their algorithms compute, bit for bit, what they computed before they shared module_core.py: every digest of
tools/record_module_trace.py's synthetic loops (five pairings, seeds 1 and 7, B = 3, the recurrent ones also B = 1) against tests/golden/module_trace.json,
which the build before the change recorded twice with equal results.  And every constructor's state_dict() is its pure initial-state function."""
import pytest
import torch

from test_module_core import GOLDEN, REC, pure_initial_state

pytestmark = pytest.mark.gpu


def leaves(tree, path=""):
    if isinstance(tree, dict):
        return {p: v for k in tree for p, v in leaves(tree[k], f"{path}/{k}").items()}
    if isinstance(tree, list):
        return {p: v for i, x in enumerate(tree) for p, v in leaves(x, f"{path}[{i}]").items()}
    return {path: tree}


def test_every_digest_is_the_parent_builds():
    got, want = leaves(REC.record()), leaves(GOLDEN)
    assert sorted(got) == sorted(want)
    assert len(want) == 16 * (12 + 3 + 2) + 16 * 5 + 12 * 2                  # per trace: actions, updates, init, final; between; the hidden states of the recurrent ones
    wrong = sorted(p for p in want if got[p] != want[p])
    assert not wrong, f"{len(wrong)} of {len(want)} digests differ, the first: {wrong[:8]}"


@pytest.mark.parametrize("seed", REC.SEEDS)
@pytest.mark.parametrize("pairing", REC.PAIRINGS)
def test_constructor_state_is_the_pure_initial_state(pairing, seed):
    policy, _ = REC.build(pairing, seed, torch.device("cuda:0"))
    got, want = policy.state_dict(), pure_initial_state(pairing, seed)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].device.type == "cpu" and got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
