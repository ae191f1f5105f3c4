"""profiles/dzfree_errors.txt from the JSONL that tests/test_dzfree_kernels_gpu.py appends to the file named by MVF_DZFREE_ERRORS (one line per reduced
quantity that is compared with the fp64 reference):

    MVF_DZFREE_ERRORS=/tmp/dzfree_errors.jsonl python -m pytest -m gpu tests/test_dzfree_kernels_gpu.py
    python tools/dzfree_errors_table.py /tmp/dzfree_errors.jsonl > profiles/dzfree_errors.txt

The last table is the BOUNDS dictionary of tests/dzfree_cases.py: 4 x the largest measured rel_l2 per quantity, kept within [4 x 2^-24, the bound
tests/test_dzfree_gpu.py uses for the quantity].
"""
import collections
import json
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import dzfree_cases as K  # noqa: E402


def family(case):
    """A case's name without the G block, the running-statistics leg and the split / row counts of the partial sums: the rows of table 2."""
    return re.sub(r" block\(\d+,\d+\)$|_(both|none|mean_only|var_only|both_momentum1)$|_split\d+_rows\d+_\d+$", "", case)


def main(path):
    rows = [json.loads(line) for line in open(path)]
    print("dz3-free / Gram glue kernels (csrc/bn_dzfree.hip) against the fp64 reference: measured rel_l2 of every reduced quantity")
    print("=" * 118)
    print("tests/test_dzfree_kernels_gpu.py on an MI355X.  Reference: tests/dzfree_ref.py on the operands as the kernels read them.  rel_l2 = helpers.rel_l2,")
    print("rel_err = helpers.rel_err (max |got - ref| / max |ref|).  G_block: one 32 x 32 block of the G part of mvf_bn_bwd_dzfree_prep's operand (bf16: one")
    print("output rounding, 2^-9 / sqrt(3) = 1.1e-3 on its own); bias: its bias vector; dw: the corrected weight gradient; dgamma / dbeta: mvf_bn_bwd_dzfree_sums;")
    print("gram_*: the outputs of mvf_bn_train_stats_gram.  Asserted: rel_l2 <= bound = 4 x the largest measured figure of the quantity, never below")
    print("4 x 2^-24 (the result's own fp32 rounding) and never above the cap (what tests/test_dzfree_gpu.py asserts for the quantity).  A bound that")
    print("sits at its cap below 4 x max is flagged `capped`; measurements above their bound would be counted in the same column.")
    print("")
    groups = collections.OrderedDict()
    for r in rows:
        groups.setdefault(r["quantity"], []).append(r)
    print("1. Per quantity (%d measurements)" % len(rows))
    print("")
    print("%-18s %6s %11s %11s %9s %11s %-14s %s" % ("quantity", "n", "max rel_l2", "4 x max", "cap", "bound", "", "worst case (rel_err)"))
    bounds = collections.OrderedDict()
    for q, g in groups.items():
        w = max(g, key=lambda r: r["rel_l2"])
        b = min(max(4 * w["rel_l2"], K.FLOOR), K.CAPS[q])
        bounds[q] = b
        over = sum(1 for r in g if r["rel_l2"] > b)
        flag = "%d ABOVE CAP" % over if over else ("capped" if 4 * w["rel_l2"] > K.CAPS[q] else "")
        print("%-18s %6d %11.3g %11.3g %9.3g %11.3g %-14s %s (%.3g)" % (q, len(g), w["rel_l2"], 4 * w["rel_l2"], K.CAPS[q], b, flag, w["case"], w["rel_err"]))
    print("")
    print("2. Per case (the worst G block of a case; the worst running-statistics leg of a Gram case; the worst split and row-count pair of a sums case)")
    print("")
    print("%-44s %-18s %4s %11s %11s" % ("case", "quantity", "n", "max rel_l2", "max rel_err"))
    cases = collections.OrderedDict()
    for r in rows:
        cases.setdefault((family(r["case"]), r["quantity"]), []).append(r)
    for (c, q), g in cases.items():
        print("%-44s %-18s %4d %11.3g %11.3g" % (c, q, len(g), max(r["rel_l2"] for r in g), max(r["rel_err"] for r in g)))
    print("")
    print("3. BOUNDS of tests/dzfree_cases.py")
    print("")
    for q, b in bounds.items():
        print('    "%s": %.2e,' % (q, b))


if __name__ == "__main__":
    main(sys.argv[1])
