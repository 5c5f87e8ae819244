"""Derives the Chebyshev tables of the formulas' i0e and i1e (include/nonlin_hip.h: NLH_EXPR_I0E, NLH_EXPR_I1E) and the
Bernoulli terms of digamma with mpmath at 40 digits, and prints them as hex-float literals: the one run whose output stands
in nonlin_amd/csrc/nlh_kernels_specfun2.h and in tests/specfun2_restatement.py.  Needs mpmath (1.3.0 made the tables).

Five functions, each expanded in Chebyshev polynomials T_k(y/2) on y in [-2, 2]:
  I0E_A   f(y) = exp(-x) I0(x),            x = 2 (y + 2)        (0 <= x <= 8)
  I0E_B   f(y) = sqrt(x) exp(-x) I0(x),    x = 32 / (y + 2)     (x >= 8; y = -2 is x = infinity)
  I1E_A   f(y) = exp(-x) I1(x) / x,        x = (y + 2) / 4      (0 <= x <= 1)
  I1E_M   f(y) = exp(-x) I1(x),            x = 4.5 + 1.75 y     (1 <= x <= 8)
  I1E_B   f(y) = sqrt(x) exp(-x) I1(x),    x = 32 / (y + 2)
i1e has three ranges where i0e has two.  exp(-x) I1(x) / x falls from 0.5 to 0.017 over [0, 8], so its series there, a sum
of terms of the size of the largest value, cancels to a thirtieth of them at x = 8 and the product with x carries the loss
(10 ulp near 7.8).  exp(-x) I1(x) itself stays between 0.13 and 0.22 on [1, 8], so its series does not cancel; the quotient
by x is kept where it is needed, next to the zero at x = 0, and varies by 2.4 there.
The coefficients are those of the interpolant at NODES Chebyshev-Gauss points, c_k = (2/NODES) sum_j f(2 cos th_j) cos(k th_j),
th_j = pi (j + 1/2) / NODES, truncated after the last one that is at least CUT times the largest; the tables list them
highest degree first, the order Clenshaw's recurrence reads them in, the degree-0 coefficient as it is (the recurrence ends
with 0.5 (b0 - b2), which halves it).
Run: python tests/golden/make_specfun2_tables.py"""
import mpmath as mp

mp.mp.dps = 40
NODES, CUT = 96, mp.mpf(2) ** -58


def i0e_low(y):
    x = 2 * (y + 2)
    return mp.exp(-x) * mp.besseli(0, x)


def i1e_low(y):
    x = (y + 2) / 4
    return mp.exp(-x) * mp.besseli(1, x) / x if x else mp.mpf(1) / 2


def i1e_middle(y):
    x = mp.mpf("4.5") + mp.mpf("1.75") * y
    return mp.exp(-x) * mp.besseli(1, x)


def high(nu):
    def f(y):
        x = 32 / (y + 2)
        return mp.sqrt(x) * mp.exp(-x) * mp.besseli(nu, x)
    return f


def chebyshev(f):
    th = [mp.pi * (j + mp.mpf(1) / 2) / NODES for j in range(NODES)]
    fy = [f(2 * mp.cos(t)) for t in th]
    c = [2 * mp.fsum(v * mp.cos(k * t) for v, t in zip(fy, th)) / NODES for k in range(NODES // 2)]
    top = max(abs(v) for v in c)
    last = max(k for k, v in enumerate(c) if abs(v) >= CUT * top)
    return c[:last + 1][::-1]


def tables():
    out = {"I0E_A": chebyshev(i0e_low), "I0E_B": chebyshev(high(0)), "I1E_A": chebyshev(i1e_low), "I1E_M": chebyshev(i1e_middle),
           "I1E_B": chebyshev(high(1))}
    # digamma(a) ~ log(a) - 1/(2a) - sum_k B_2k / (2k a^2k): the terms B_2k / (2k), k = 1 .. 7
    out["DIGAMMA_B"] = [mp.bernoulli(2 * k) / (2 * k) for k in range(1, 8)]
    return out


def main():
    for name, c in tables().items():
        print(f"{name} [{len(c)}]")
        vals = [float(v).hex() for v in c]
        for i in range(0, len(vals), 4):
            print("    " + ", ".join(vals[i:i + 4]) + ",")


if __name__ == "__main__":
    main()
