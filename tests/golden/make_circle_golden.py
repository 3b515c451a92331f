"""Writes tests/golden/circle_golden.json: vectors of the circle transform over Mersenne31 computed STRAIGHT from the
definition (include/sppark_amd_circle.h; tests/circle_model.py domain_direct / direct_evaluate, Python integers,
O(n^2)) for k = 1 ... 6 in both evaluation orders, and the header's anchors.

    python tests/golden/make_circle_golden.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import circle_model as M  # noqa: E402


def main():
    rnd = random.Random(0xC19C1E)
    cases = []
    for k in range(1, 7):
        n = 1 << k
        c = [rnd.randrange(M.P) for _ in range(n)]
        c[rnd.randrange(n)] = M.P - 1
        nat = M.direct_evaluate(c, k)
        cases.append({"lg": k, "coefficients": c, "domain_natural": [list(p) for p in M.domain_direct(k)],
                      "evals_natural": nat, "evals_bitrev": [nat[M.bitrev(q, k)] for q in range(n)]})
    out = {"modulus": M.P, "generator": list(M.G),
           "anchors": {"g_2": list(M.g_of_order(2)), "g_3": list(M.g_of_order(3)),
                       "evals_1234_lg2": M.direct_evaluate([1, 2, 3, 4], 2),
                       "evals_1to8_lg3": M.direct_evaluate(list(range(1, 9)), 3)},
           "cases": cases}
    with open(os.path.join(HERE, "circle_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
