#!/usr/bin/env python3
"""Coefficients of the dilogarithm's core polynomial (gwinferno_amd/csrc/gwi_spinprior.h: li2_core; gwinferno_amd/spin_priors.py: LI2_COEFS).

Re Li2(x) for every real x is reduced to x in [0, 1/2] (inversion for |x| > 1, reflection for (1/2, 1], Landen's map for [-1, 0));
there Li2(x) = x P(x) with P a polynomial of degree d for Li2(x)/x = sum_k x^(k-1)/k^2.  P is the interpolant of Li2(x)/x at the
d + 1 Chebyshev points of [0, 1/2] (50-digit arithmetic, mpmath): the nearest singularity, x = 1, maps to t = 3 on the Chebyshev
variable, so the error falls like (3 + sqrt 8)^-d and the interpolant is within a small factor of the minimax polynomial.  The low
coefficients are close to 1/k^2; the high ones are not -- at degree 20 those of x^11 and up alternate in sign, the largest 9.47 at
x^17 -- but on [0, 1/2] such a term is at most 9.47 / 2^17 = 7e-5 of a sum that is at least 1, so Horner's rule loses nothing that
matters to their cancellation.  The script prints the coefficients rounded to double, highest degree LAST, and the largest relative
error of x P(x) -- with the rounded coefficients, exact arithmetic -- on a fine grid.  The committed coefficients are degree 20
(3.07e-18).      python tools/li2_poly.py [degree=20]"""
import sys

import mpmath as mp

mp.mp.dps = 60
HALF = mp.mpf(1) / 2


def target(x):
    return mp.polylog(2, x) / x if x != 0 else mp.mpf(1)


def interpolant(degree):
    n = degree + 1
    nodes = [HALF / 2 * (1 + mp.cos(mp.pi * (2 * k + 1) / (2 * n))) for k in range(n)]
    A = mp.matrix(n, n)
    b = mp.matrix(n, 1)
    for i, x in enumerate(nodes):
        for j in range(n):
            A[i, j] = x**j
        b[i] = target(x)
    return [mp.lu_solve(A, b)[j] for j in range(n)]


def error(coefs, n_grid=2001):
    worst = mp.mpf(0)
    rounded = [mp.mpf(float(c)) for c in coefs]
    for i in range(1, n_grid):
        x = HALF * i / (n_grid - 1)
        p = mp.mpf(0)
        for c in reversed(rounded):
            p = p * x + c
        worst = max(worst, abs(p * x / mp.polylog(2, x) - 1))
    return worst


def main():
    degree = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    coefs = interpolant(degree)
    print(f"# degree {degree}: max relative error of x P(x) on (0, 1/2] = {mp.nstr(error(coefs), 3)}")
    for j, c in enumerate(coefs):
        print(f"    {float(c)!r},  # x^{j}")


if __name__ == "__main__":
    main()
