"""A HAND-COMPUTED known-answer vector for the LAMB update of msa_amd.optim.LAMB (You et al., "Large Batch Optimization for Deep
Learning", Algorithm 2 with bias correction; apex FusedLAMB's defaults).

The numbers below were obtained by evaluating the PUBLISHED rule

    m_t = b1 m_{t-1} + (1 - b1) g_t                     v_t = b2 v_{t-1} + (1 - b2) g_t^2
    u   = (m_t / (1 - b1^t)) / (sqrt(v_t / (1 - b2^t)) + eps) + wd p
    r   = ||p|| / ||u||  over the tensor (1 when wd = 0: the tensor takes the plain Adam step)
    p  <- p - lr r u

in 60-digit decimal arithmetic, scalar by scalar (no tensor library, no optimizer implementation), with lr = 0.1, b1 = 0.9,
b2 = 0.999, eps = 1e-6.  First step of tensor "w" by hand: mhat = g, vhat = g^2, so mhat / (sqrt(vhat) + eps) is the sign of g less
2e-6 .. 8e-6; u = (1.009998, -1.004996, 1.002492), ||u|| = 1.7421547..., ||p|| = sqrt(1.3125) = 1.1456439..., r = 0.6576017...,
p_1[0] = 1 - 0.1 x 0.6576017 x 1.009998 = 0.9335823...

Each tensor: (weight decay, p0, [g_1, g_2, g_3], [p_1, p_2, p_3], [r_1..3], [||p||_1..3] (before each step), [||u||_1..3], m_3, v_3).
"w" decays (three elements, a zero gradient element at step 2); "b" has weight decay 0 and so ratio 1 (two elements, eps-scale second
moments and a zero gradient at step 2).  Used by tests/test_lamb_reference_cpu.py."""

LR, BETA1, BETA2, EPS = 0.1, 0.9, 0.999, 1e-6

TENSORS = {
    "w": (0.01, [1.0, -0.5, 0.25],
          [[0.5, -0.25, 0.125], [-0.1, 0.2, 0.0], [0.3, 0.3, -0.6]],
          [[0.9335823594412853503085474, -0.4339112918127121917315698, 0.1840759552761748380321768],
           [0.8697180102786330811916847, -0.4262450360735300085723805, 0.1016140652159415850651345],
           [0.7999211601446930527271085, -0.4677080327335230705975696, 0.1554045502821157928872022]],
          [0.6576017037504194021773577, 1.227309744570943613608378, 1.036712928258433921043157],
          [1.145643923738960001647012, 1.045819768570746759416294, 0.9738684030350605053673242],
          [1.742154737746494681518238, 0.8521237390943684649637010, 0.9393809766326099062814124],
          [0.0615, 0.02775, -0.049875],
          [0.00034949025, 0.0001923350625, 0.000375593765625]),
    "b": (0.0, [-2.0, 0.75],
          [[0.001, -0.002], [0.0, 0.004], [-0.002, 0.001]],
          [[-2.099900099900099900099900, 0.8499500249875062468765617],
           [-2.166811274945140338875296, 0.8133512440981311191831634],
           [-2.132834138584734448223450, 0.7718018294359183120185290]],
          [1.0, 1.0, 1.0],
          [2.136000936329382791967912, 2.265390799517097013388873, 2.314435427378643076970877],
          [1.413153829384935120341080, 0.7626648089755113662790326, 0.5367308127940970610646853],
          [-0.000119, 0.000298],
          [4.998001e-9, 2.0976004e-8]),
}
