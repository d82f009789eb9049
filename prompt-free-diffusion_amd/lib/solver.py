"""DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2: multistep, data prediction) on the host, in fp64 -- numpy only.

The device evaluates one row of `dpmpp_2m_table` per step inside the fused step kernel (pfd_cfg_dpmpp_step); this
module is the specification restated, the oracle of the tests, and where the sampler's coefficient table comes from.

The schedule is the DDIM sampler's own, unchanged: step `i` (rows are indexed like ddim_alphas, so a run walks
i = n-1 ... 0) goes from a_t = alphas[i] to its target a_s = alphas_prev[i]; the last step (row 0) targets
alphas_cumprod[0] exactly as DDIM does.  With lambda(a) = 0.5 log(a / (1 - a)) (half the log signal-to-noise ratio):

    h    = lambda(a_s) - lambda(a_t)
    c_x  = sqrt((1 - a_s) / (1 - a_t))
    c_d  = -sqrt(a_s) expm1(-h)
    x0   = (x - sqrt(1 - a_t) e) / sqrt(a_t)                      e: the guided eps
    D    = x0                                                     first-order step
    D    = w_cur x0 + w_prev x0_last,  r = h_last / h,            second-order step
           w_prev = -1 / (2 r),  w_cur = 1 - w_prev
    x_next = c_x x + c_d D

First-order steps: the first of a run (no history), the last (row 0), and every step at order = 1.  A first-order
step is DDIM at eta = 0: c_x x + c_d x0 = sqrt(a_s) x0 + sqrt(1 - a_s) e.
"""
import numpy as np

SOLVERS = ('ddim', 'dpmpp_2m', 'dpmpp_1')


def solver_order(solver):
    """None for 'ddim' (the DDIM kernels), else the order the multistep kernel runs at; an unknown name raises"""
    if solver not in SOLVERS:
        raise ValueError(f"unknown solver {solver!r}: one of {', '.join(SOLVERS)}")
    return {'ddim': None, 'dpmpp_2m': 2, 'dpmpp_1': 1}[solver]


def half_log_snr(a):
    a = np.asarray(a, dtype=np.float64)
    return 0.5 * np.log(a / (1.0 - a))


def dpmpp_2m_table(alphas, alphas_prev, scale, order=2):
    """fp64 [n, 8] rows {a_t, sqrt(1-a_t), c_x, c_d, w_cur, w_prev, scale, 0}; row i is the step alphas[i] ->
    alphas_prev[i], its history the step of row i + 1.  Rows 0 and n-1, and every row at order = 1, are first-order:
    w_cur = 1, w_prev = 0."""
    if order not in (1, 2):
        raise ValueError(f"order must be 1 or 2: got {order!r}")
    a_t = np.asarray(alphas, dtype=np.float64)
    a_s = np.asarray(alphas_prev, dtype=np.float64)
    if a_t.ndim != 1 or a_t.shape != a_s.shape or a_t.size == 0:
        raise ValueError("alphas and alphas_prev must be two vectors of one length")
    n = a_t.shape[0]
    h = half_log_snr(a_s) - half_log_snr(a_t)
    w_cur, w_prev = np.ones(n), np.zeros(n)
    if order == 2 and n > 2:
        r = h[2:] / h[1:-1]                  # h_last / h for rows 1 .. n-2
        w_prev[1:-1] = -1.0 / (2.0 * r)
        w_cur[1:-1] = 1.0 - w_prev[1:-1]
    tab = np.zeros((n, 8))
    tab[:, 0] = a_t
    tab[:, 1] = np.sqrt(1.0 - a_t)
    tab[:, 2] = np.sqrt((1.0 - a_s) / (1.0 - a_t))
    tab[:, 3] = -np.sqrt(a_s) * np.expm1(-h)
    tab[:, 4] = w_cur
    tab[:, 5] = w_prev
    tab[:, 6] = float(scale)
    return tab


def dpmpp_2m_run(eps_fn, x_T, alphas, alphas_prev, order=2):
    """the whole loop in fp64: `eps_fn(x, i)` is the (guided) eps at a_t = alphas[i]; -> x after the step of row 0"""
    tab = dpmpp_2m_table(alphas, alphas_prev, 1.0, order)
    n = tab.shape[0]
    x = np.asarray(x_T, dtype=np.float64)
    x0_last = None
    for i in range(n - 1, -1, -1):
        a_t, s1m, c_x, c_d, w_cur, w_prev = tab[i, :6]
        e = np.asarray(eps_fn(x, i), dtype=np.float64)
        x0 = (x - s1m * e) / np.sqrt(a_t)
        d = x0 if (x0_last is None or w_prev == 0.0) else w_cur * x0 + w_prev * x0_last
        x = c_x * x + c_d * d
        x0_last = x0
    return x
