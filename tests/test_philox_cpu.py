"""CPU: the NumPy restatement of the device generator (tests/philox_restatement.py) is Philox4x32-10 (the known answers of the
Random123 distribution, tests/golden/philox_kat.json), its normals are standard normal to the bars of
test_philox_randn_statistics (tests/test_gpu_sapg_fista.py), and every word of the counter and of the key reaches the output.
tests/test_gpu_philox.py holds the device to this restatement."""
import json
import math
import os

import numpy as np

from conftest import GOLDEN

import philox_restatement as pr


def test_known_answers_of_philox4x32_10():
    with open(os.path.join(GOLDEN, "philox_kat.json")) as f:
        vectors = json.load(f)["vectors"]
    assert len(vectors) == 3
    for v in vectors:
        words = lambda k: [np.uint64(int(w, 16)) for w in v[k]]
        out = pr.philox4x32_10(words("counter"), words("key"))
        assert [f"{int(o[0]):08x}" for o in out] == v["output"], v
    # vectorised: the three vectors in one call give the three answers
    cols = lambda k, n: [np.array([int(v[k][i], 16) for v in vectors], dtype=np.uint64) for i in range(n)]
    out = pr.philox4x32_10(cols("counter", 4), cols("key", 2))
    for i, v in enumerate(vectors):
        assert [f"{int(o[i]):08x}" for o in out] == v["output"]


def test_normal_pairs_of_the_third_vector_by_hand():
    """The mapping words -> normals written out in Python floats on the third known answer (counter q = c1 << 32 | c0)."""
    c = [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]
    o = [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    seed = (0x299f31d0 << 32) | 0xa4093822
    z0, z1 = pr.normal_pairs(np.array([(c[1] << 32) | c[0]], dtype=np.uint64), c[2], c[3], seed)
    a, b = (o[0] << 32) | o[1], (o[2] << 32) | o[3]
    u1, u2 = ((a >> 11) + 0.5) * 2.0 ** -53, ((b >> 11) + 0.5) * 2.0 ** -53
    r = math.sqrt(-2.0 * math.log(u1))
    assert abs(z0[0] - r * math.cos(2 * math.pi * u2)) <= 8 * np.spacing(r)
    assert abs(z1[0] - r * math.sin(2 * math.pi * u2)) <= 8 * np.spacing(r)


def test_sincos_reduction_is_exact_at_the_quadrants():
    s, c = pr._sincos_2pi(np.array([0.0, 0.125, 0.25, 0.5, 0.75, 1.0]))
    np.testing.assert_array_equal(s[[0, 2, 3, 4, 5]], [0.0, 1.0, 0.0, -1.0, 0.0])
    np.testing.assert_array_equal(c[[0, 2, 3, 4, 5]], [1.0, 0.0, -1.0, 0.0, 1.0])
    assert abs(s[1] - math.sqrt(0.5)) <= 1.2e-16 and abs(c[1] - math.sqrt(0.5)) <= 1.2e-16
    u = np.random.default_rng(0).random(1000)
    s, c = pr._sincos_2pi(u)
    assert np.max(np.abs(s - np.sin(2 * np.pi * u))) < 1e-15 and np.max(np.abs(c - np.cos(2 * np.pi * u))) < 1e-15


def test_normals_are_standard_normal():
    """2^20 pairs of one step: the bars of test_philox_randn_statistics (65 536 values there, 2 097 152 here)."""
    z0, z1 = pr.normal_pairs(np.arange(1 << 20, dtype=np.uint64), 0, 3, (7 << 32) | 5)
    Z = np.stack([z0, z1], axis=1).ravel()                         # device order
    assert np.all(np.isfinite(Z))
    print(f"mean {Z.mean():.2e}, var - 1 {Z.var() - 1:.2e}, skew {np.mean(Z ** 3):.2e}, kurt - 3 {np.mean(Z ** 4) - 3:.2e}, "
          f"lag-1 {np.corrcoef(Z[:-1], Z[1:])[0, 1]:.2e}, pair {np.corrcoef(z0, z1)[0, 1]:.2e}")
    assert abs(Z.mean()) < 4 / math.sqrt(Z.size)
    assert abs(Z.var() - 1) < 0.03
    assert abs(np.mean(Z ** 3)) < 0.05 and abs(np.mean(Z ** 4) - 3) < 0.15
    assert abs(np.corrcoef(Z[:-1], Z[1:])[0, 1]) < 0.01
    assert abs(np.corrcoef(z0, z1)[0, 1]) < 0.01


def test_every_counter_and_key_word_changes_the_output():
    q = np.arange(64, dtype=np.uint64)
    base = dict(q=q, step=2, chain=3, seed=(7 << 32) | 5)
    z = np.stack(pr.normal_pairs(**base))
    others = dict(q_lo=dict(base, q=q + np.uint64(64)), q_hi=dict(base, q=q + (np.uint64(1) << np.uint64(32))),
                  step=dict(base, step=3), chain=dict(base, chain=4), seed_lo=dict(base, seed=(7 << 32) | 4),
                  seed_hi=dict(base, seed=(6 << 32) | 5), seed_hi_dropped=dict(base, seed=5),
                  step_chain_swapped=dict(base, step=3, chain=2))
    seen = [z]
    for name, kw in others.items():
        w = np.stack(pr.normal_pairs(**kw))
        for s in seen:                                             # no two of the streams share a single value
            assert not np.any(w == s), name
        seen.append(w)
    np.testing.assert_array_equal(np.stack(pr.normal_pairs(**base)), z)


def test_chain_normals_layout_and_reshaping():
    """Pair q fills doubles 2q, 2q + 1; chain b draws chain_offset + b; step numbers count from 0; as_arrays gives the (M, C)
    array whose column-major storage is the device order."""
    seed = (7 << 32) | 5
    z = pr.chain_normals(12, 3, 2, seed, chain_offset=3)
    assert z.shape == (3, 2, 12)
    for s in range(3):
        for b in range(2):
            z0, z1 = pr.normal_pairs(np.arange(6, dtype=np.uint64), s, 3 + b, seed)
            np.testing.assert_array_equal(z[s, b, 0::2], z0)
            np.testing.assert_array_equal(z[s, b, 1::2], z1)
    np.testing.assert_array_equal(pr.chain_normals(12, [2], 1, seed, chain_offset=4)[0, 0], z[2, 1])
    a = pr.as_arrays(z, 4)
    assert a.shape == (3, 2, 4, 3)
    np.testing.assert_array_equal(a[1, 1].ravel(order="F"), z[1, 1])
    np.testing.assert_array_equal(pr.device_order(a), z)
