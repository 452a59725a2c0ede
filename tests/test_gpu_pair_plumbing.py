"""register_pairs checks the class of `out=` like every other one-call entry point: a result object of another entry point is refused
with the ValueError they all give (it used to end in an AttributeError), its own earlier result is taken and filled again."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_BLOCKS, K, C, MAX_ITERATION, MAX_VALIDATION = 2, 8, 16, 64, 4


def test_register_pairs_refuses_the_result_of_another_entry_point(device):
    from d3feat_amd import registration as reg
    rng = np.random.default_rng(3)
    # two blocks of the same 8 points, the second one rotated and shifted, with the same unit descriptors: every row has its twin
    base, desc = rng.uniform(-1, 1, (K, 3)), rng.standard_normal((K, C))
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    score = np.linspace(0.1, 0.9, K)[:, None]
    blocks = [np.concatenate([xyz, desc, score], 1).astype(np.float32) for xyz in (base, base @ q.T + 0.25)]
    kp, count = reg.stack_keypoints(blocks, K, device=device)
    assert tuple(kp.shape) == (N_BLOCKS, K, 4 + C)
    pairs = torch.tensor([(0, 1)], dtype=torch.int32, device=device)                # P = 1
    kw = dict(max_correspondence_distance=0.05, ransac_n=3, max_iteration=MAX_ITERATION, max_validation=MAX_VALIDATION, seed=1)

    counts = reg.register_pairs_counts(kp, count, pairs, num_keypts=(K,), **kw)
    assert isinstance(counts, reg.PairRegistrationCounts)
    with pytest.raises(ValueError, match="register_pairs: out= was made for another call"):
        reg.register_pairs(kp, count, pairs, out=counts, **kw)

    first = reg.register_pairs(kp, count, pairs, **kw)
    assert int(first.mutual_count[0]) == K and int(first.validations[0]) == MAX_VALIDATION      # the call did register something
    want = {f: getattr(first, f).clone() for f in first.FIELDS if getattr(first, f) is not None}
    host = first.host(0)
    for f in want:
        getattr(first, f).fill_(-7)                                                 # the second call has to write every tensor again
    again = reg.register_pairs(kp, count, pairs, out=first, **kw)
    assert again is first
    for f, t in want.items():
        assert torch.equal(getattr(again, f), t), f
    got = again.host(0)                                                             # a new read-back, not the one of the first call
    assert sorted(got) == sorted(host) and all(np.array_equal(got[k], host[k]) for k in host)
    assert np.array_equal(got["transformation"][:3], first.T[0].cpu().numpy().astype(np.float64))
