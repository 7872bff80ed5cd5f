"""CPU: the float64 LAMB reference (tests/lamb_ref.py) is what it says -- it reproduces the hand-computed vector
tests/golden/lamb_hand.py, gives ratio 1 where the rule says 1, and caps at max_trust."""
import numpy as np

from tests import lamb_ref as L
from tests.golden import lamb_hand as G

HYPER = [(G.LR, G.BETA1, G.BETA2, G.EPS, G.TENSORS["w"][0]), (G.LR, G.BETA1, G.BETA2, G.EPS, G.TENSORS["b"][0])]


def test_reference_reproduces_the_hand_computed_vector():
    w, b = G.TENSORS["w"], G.TENSORS["b"]
    tensors = [(0, 3, 0), (4, 2, 1)]                                      # (element 3 and 6, 7 belong to no tensor)
    P = np.array(w[1] + [7.0] + b[1] + [7.0, 7.0])
    M, V = np.zeros(8), np.zeros(8)
    for t in range(3):
        g = np.array(w[2][t] + [9.0] + b[2][t] + [9.0, 9.0])
        out = L.lamb_step(P, g, M, V, tensors, HYPER, t + 1)
        P, M, V = out["P"], out["M"], out["V"]
        for k, (x, s) in enumerate(((w, slice(0, 3)), (b, slice(4, 6)))):
            np.testing.assert_allclose(P[s], x[3][t], rtol=1e-13, atol=0)
            np.testing.assert_allclose(out["R"][k], x[4][t], rtol=1e-13)
            np.testing.assert_allclose(out["NP"][k], x[5][t], rtol=1e-13)
            np.testing.assert_allclose(out["NU"][k], x[6][t], rtol=1e-13)
        assert P[3] == 7.0 and P[6] == 7.0 and M[3] == 0.0 and V[7] == 0.0
    np.testing.assert_allclose(M[0:3], w[7], rtol=1e-13)
    np.testing.assert_allclose(V[0:3], w[8], rtol=1e-13)
    np.testing.assert_allclose(M[4:6], b[7], rtol=1e-13)
    np.testing.assert_allclose(V[4:6], b[8], rtol=1e-13)
    assert out["R"][1] == 1.0                                             # wd = 0: exactly the Adam step


def test_ratio_is_one_for_a_zero_tensor_a_zero_update_and_no_decay():
    h = [(1e-2, 0.9, 0.999, 1e-6, 0.1), (1e-2, 0.9, 0.999, 1e-6, 0.0)]
    rng = np.random.default_rng(0)
    P, Gd, M, V = rng.normal(size=32), rng.normal(size=32), 0.1 * rng.normal(size=32), rng.uniform(size=32)
    P[0:8] = 0.0; Gd[0:8] = 0.0; M[0:8] = 0.0; V[0:8] = 0.0               # tensor 0: all zero (||p|| = ||u|| = 0)
    Gd[8:16] = 0.0; M[8:16] = 0.0                                         # tensor 1: g = m = 0, wd = 0 -> u = 0, ||p|| > 0
    tensors = [(0, 8, 0), (8, 8, 1), (16, 8, 1), (24, 8, 0)]              # tensor 2: wd = 0, u != 0; tensor 3: adapts
    out = L.lamb_step(P, Gd, M, V, tensors, h, 3)
    assert out["R"][0] == 1.0 and out["R"][1] == 1.0 and out["R"][2] == 1.0
    assert out["NU"][1] == 0.0 and out["NP"][1] > 0.0 and out["NU"][2] > 0.0
    assert np.array_equal(out["P"][0:16], P[0:16])                        # nothing to apply
    want = out["NP"][3] / out["NU"][3]
    assert out["R"][3] == want and abs(want - 1.0) > 1e-3
    np.testing.assert_allclose(out["P"][24:], P[24:] - 1e-2 * want * out["U"][24:], rtol=1e-15)
    # always_adapt: the no-decay tensor with an update adapts too; the zero ones stay at 1
    out2 = L.lamb_step(P, Gd, M, V, tensors, h, 3, always_adapt=True)
    assert out2["R"][0] == 1.0 and out2["R"][1] == 1.0 and out2["R"][2] == out2["NP"][2] / out2["NU"][2] != 1.0
    # a decay flag that is off turns a decaying group's tensor into a plain Adam one
    out3 = L.lamb_step(P, Gd, M, V, tensors, h, 3, decay=[True, True, True, False])
    assert out3["R"][3] == 1.0 and np.array_equal(out3["A"][24:], np.abs(out3["U"][24:]))


def test_max_trust_caps_the_ratio():
    h = [(1e-2, 0.9, 0.999, 1e-6, 0.1)]
    rng = np.random.default_rng(1)
    P, Gd = 50.0 * rng.normal(size=16), rng.normal(size=16)
    free = L.lamb_step(P, Gd, np.zeros(16), np.zeros(16), [(0, 16, 0)], h, 1)
    assert free["R"][0] > 10.0
    cap = L.lamb_step(P, Gd, np.zeros(16), np.zeros(16), [(0, 16, 0)], h, 1, max_trust=10.0)
    assert cap["R"][0] == 10.0
    np.testing.assert_allclose(cap["P"], P - 1e-2 * 10.0 * cap["U"], rtol=1e-15)
    loose = L.lamb_step(P, Gd, np.zeros(16), np.zeros(16), [(0, 16, 0)], h, 1, max_trust=1e6)
    assert loose["R"][0] == free["R"][0]


def test_the_scales_of_the_bounds():
    h = [(1e-2, 0.9, 0.999, 1e-6, 0.5)]
    P, Gd = np.array([2.0, -2.0, 0.0, 0.0]), np.array([-1.0, 1.0, 0.0, 0.0])
    out = L.lamb_step(P, Gd, np.zeros(4), np.zeros(4), [(0, 4, 0)], h, 1)
    # mhat / (sqrt(vhat) + eps) = -+1 (less 1e-6), wd p = +-1: the terms cancel, a stays 2
    assert np.all(np.abs(out["U"][:2]) < 2e-6) and np.allclose(out["A"][:2], 2.0, atol=2e-6) and out["CANCEL"][0] > 1e5
    c = L.coefs(h[0], 2, f32=True)
    assert c[0] == float(np.float32(0.9)) and c[5] == float(np.float32(1.0 / (1.0 - 0.81)))
