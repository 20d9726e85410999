"""Host restatement of slice_chain_kernel's sampler arithmetic (csrc/slice.hip), operation by operation: Python floats, explicit
loops, one rounding per operation, no fused operations and no library norm.  It is samplers/slice.lua:51-168 in its default mode
(random direction, log space, step-out, per-dimension widths, max_step) plus what the kernel adds: the bounds (a request outside
them is -inf and not evaluated), the memo (an update starts from the known value of the point the last one ended on), the
evaluation cap and the stop on a failed pivot.  The density and the draws come from the caller.

Also here: the library's counter generator (csrc/counter_rng.h) and the kernel's counter layout, on the host."""
import math

import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
KIND_START, KIND_RIGHT, KIND_LEFT, KIND_SHRINK = 0, 1, 2, 3
ST_NAN, ST_ZERO, ST_CAP, ST_PIVOT, ST_NOT_RUN = 1, 2, 4, 8, 16
# update g owns the counters 4096 g .. 4096 g + 4095
CTR_STRIDE, CTR_Z, CTR_UY, CTR_RIGHT, CTR_SHRINK = 4096, 0, 64, 128, 256


def splitmix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def counter_key(seed, stream):
    return splitmix64(splitmix64(seed) ^ stream)


def counter_bits(key, ctr):
    """The two 64-bit words a counter owns: (a, b) of counter_normal; a alone is counter_uniform's."""
    return splitmix64(key + GAMMA * (2 * ctr + 1)), splitmix64(key + GAMMA * (2 * ctr + 2))


def counter_uniform(key, ctr):
    return float(counter_bits(key, ctr)[0] >> 11) * 2.0 ** -53


def counter_normal(key, ctr):
    """Box-Muller on the counter's two words, with numpy's log / cos (the device's are ocml's: a few ulp apart)."""
    a, b = counter_bits(key, ctr)
    u1 = float((a >> 11) + 1) * 2.0 ** -53
    u2 = float(b >> 11) * 2.0 ** -53
    return float(np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925 * u2))


class CounterDraws(object):
    """The draws of chain `chain` of a call with `seed`, by the kernel's layout."""

    def __init__(self, seed, chain):
        self.key = counter_key(seed, chain)

    def normals(self, g, D):
        return [counter_normal(self.key, CTR_STRIDE * g + CTR_Z + k) for k in range(D)]

    def u_Y(self, g):
        return counter_uniform(self.key, CTR_STRIDE * g + CTR_UY)

    def log_u_Y(self, g):
        u = self.u_Y(g)
        return float(np.log(u)) if u > 0.0 else -math.inf

    def u_right(self, g, D):
        return [counter_uniform(self.key, CTR_STRIDE * g + CTR_RIGHT + k) for k in range(D)]

    def u_shrink(self, g, i):
        return counter_uniform(self.key, CTR_STRIDE * g + CTR_SHRINK + i)


class _Cap(Exception):
    pass


class _Pivot(Exception):
    pass


def slice_chain(density, draws, theta0, lo, hi, widths, U, update0=0, max_step=1000, max_evals=512):
    """U updates of one chain from theta0.  density(theta list) -> value, or (value, pivot_failed).  draws: normals(g, D),
    log_u_Y(g), u_right(g, D), u_shrink(g, i), asked for in this order within an update.
    Returns {'theta': U lists, 'value': U floats, 'status': U ints, 'nevals': int, 'requests': the density requests in order,
    each {'g', 'kind', 'u', 'in_bounds', 'reused', 'theta', 'value'}}."""
    D = len(theta0)
    lo, hi, widths = [float(v) for v in lo], [float(v) for v in hi], [float(v) for v in widths]
    x0 = [float(v) for v in theta0]
    fx0, have_fx0, dead = math.nan, False, False
    out_theta, out_value, out_status, requests = [], [], [], []
    nevals = 0
    for u in range(U):
        if dead:
            out_theta.append(list(x0)), out_value.append(fx0), out_status.append(ST_NOT_RUN)
            continue
        g = update0 + u
        z = [float(v) for v in draws.normals(g, D)]
        ss = 0.0
        for k in range(D):
            sq = z[k] * z[k]
            ss = ss + sq
        nrm = math.sqrt(ss)
        direction = [z[k] / nrm for k in range(D)]
        luY = float(draws.log_u_Y(g))
        ur = [float(v) for v in draws.u_right(g, D)]
        right = [ur[k] * widths[k] for k in range(D)]
        left = [right[k] - widths[k] for k in range(D)]
        status, nreq, started = 0, 0, False

        def ask(kind, theta, us=0.0):
            nonlocal nreq, nevals
            if nreq >= max_evals:
                raise _Cap()
            nreq += 1
            inb = all(theta[k] >= lo[k] and theta[k] <= hi[k] for k in range(D))   # a NaN fails both comparisons
            reused = kind == KIND_START and have_fx0
            piv = False
            if reused:
                v = fx0
            elif not inb:
                v = -math.inf
            else:
                v = density(list(theta))
                if isinstance(v, tuple):
                    v, piv = v
                v = float(v)
                nevals += 1
            requests.append({"g": g, "kind": kind, "u": us, "in_bounds": inb, "reused": reused, "theta": list(theta), "value": v})
            if piv:
                raise _Pivot()
            return v

        def along(dx):
            th = []
            for k in range(D):
                mv = direction[k] * dx[k]
                th.append(x0[k] + mv)
            return th

        try:
            f0 = ask(KIND_START, list(x0))
            fx0, started = f0, True
            Y = f0 + luY
            itr = 0
            while True:
                v = ask(KIND_RIGHT, along(right))
                if v > Y and itr < max_step:
                    itr += 1
                    right = [right[k] + widths[k] for k in range(D)]
                else:
                    break
            itr = 0
            while True:
                v = ask(KIND_LEFT, along(left))
                if v > Y and itr < max_step:
                    itr += 1
                    left = [left[k] - widths[k] for k in range(D)]
                else:
                    break
            i = 0
            while True:
                us = float(draws.u_shrink(g, i))
                dx = []
                for k in range(D):
                    span = right[k] - left[k]
                    step = span * us
                    dx.append(left[k] + step)
                theta = along(dx)
                y = ask(KIND_SHRINK, theta, us)
                if y != y:
                    status |= ST_NAN
                    break
                if y > Y:
                    break
                if any(dx[k] == 0.0 for k in range(D)):
                    status |= ST_ZERO
                    break
                right = [dx[k] if dx[k] > 0.0 else right[k] for k in range(D)]
                left = [dx[k] if dx[k] < 0.0 else left[k] for k in range(D)]
                i += 1
            x0, fx0, have_fx0 = theta, y, True
            out_theta.append(list(x0)), out_value.append(fx0), out_status.append(status)
        except _Cap:
            have_fx0 = True
            out_theta.append(list(x0)), out_value.append(fx0), out_status.append(status | ST_CAP)
        except _Pivot:
            if not started:
                fx0 = math.nan
            dead = True
            out_theta.append(list(x0)), out_value.append(fx0), out_status.append(status | ST_PIVOT)
    return {"theta": out_theta, "value": out_value, "status": out_status, "nevals": nevals, "requests": requests}
