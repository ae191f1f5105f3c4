"""profiles/wgrad_errors.txt from the JSONL that tests/test_wgrad_families_gpu.py appends to the file named by MVF_WGRAD_ERRORS (one line per weight-gradient
call that is compared with the fp64 reference, in the parent process and in every forced leg's child):

    MVF_WGRAD_ERRORS=/tmp/wgrad_errors.jsonl python -m pytest -m gpu tests/test_wgrad_families_gpu.py
    python tools/wgrad_errors_table.py /tmp/wgrad_errors.jsonl > profiles/wgrad_errors.txt
"""
import collections
import json
import sys


def main(path):
    rows = [json.loads(line) for line in open(path)]
    legs = []
    for r in rows:
        r["leg"] = r["policy"] or "default"
        if r["leg"] not in legs:
            legs.append(r["leg"])
    tile = lambda r: "%dx%d" % tuple(r["tile"])                                    # noqa: E731
    print("Conv weight gradients against the fp64 reference: measured error of every case under the default policy and every forced policy")
    print("=" * 125)
    print("tests/test_wgrad_families_gpu.py on an MI355X: every in-process case under the default launch policy and again in one child process per forced policy")
    print("(LEGS).  Reference: tests/wgrad_ref.py, fp64 tap loops over the operands as stored (rounded to the storage type on the CPU), so what is measured is the")
    print("fp32 accumulation error of the kernel and of the fixed-order slab reduce.  Families as mvf_conv2d_wgrad_last_launch names them (bf16_pipe/N = N-stage ring).")
    print("")
    print("rel_err = helpers.rel_err (max |got - ref| / max |ref|), rel_l2 = helpers.rel_l2; both are asserted < bound (2e-6; the direct stem kernel 2e-5).")
    print("vs sum|dz||x| = the worst element's error against ITS OWN sum of |dz| |x| (a figure, nothing asserted).  split = the split operand (x2).")
    print("")
    print("1. Worst case per forced policy x family x tile x storage type x split operand (%d measurements, %d policies)" % (len(rows), len(legs)))
    print("")
    print("%-62s %-12s %-8s %-5s %-5s %5s %10s %10s %8s  %s" % ("policy", "family", "tile", "type", "split", "cases", "rel_err", "rel_l2", "bound", "worst shape (rel_err)"))
    groups = collections.OrderedDict()
    for r in rows:
        groups.setdefault((r["leg"], r["family"], tile(r), r["dtype"], r["split"]), []).append(r)
    for leg in legs:
        for key in sorted(k for k in groups if k[0] == leg):
            g = groups[key]
            w = max(g, key=lambda r: r["rel_err"])
            print("%-62s %-12s %-8s %-5s %-5d %5d %10.3g %10.3g %8.0e  %s" % (key + (len(g), w["rel_err"], max(r["rel_l2"] for r in g), w["bound"], w["shape"])))
    print("")
    print("2. Every case")
    print("")
    print("%-62s %-18s %-46s %-5s %-12s %-8s %11s %10s %10s %13s" % ("policy", "entry", "shape", "type", "family", "tile", "splits x rows", "rel_err", "rel_l2", "vs sum|dz||x|"))
    for leg in legs:
        for r in rows:
            if r["leg"] == leg:
                print("%-62s %-18s %-46s %-5s %-12s %-8s %5d x %-5d %10.3g %10.3g %13.3g" % (leg, r["entry"], r["shape"], r["dtype"], r["family"], tile(r), r["nsplit"], r["rows"],
                                                                                         r["rel_err"], r["rel_l2"], r["rel_abs"]))
    worst = max(rows, key=lambda r: max(r["rel_err"], r["rel_l2"]) / r["bound"])
    print("")
    print("Largest fraction of its bound: %.3g of %.0e (%s %s %s, %s, policy %s)" % (max(worst["rel_err"], worst["rel_l2"]), worst["bound"], worst["entry"], worst["shape"],
                                                                               worst["dtype"], worst["family"], worst["leg"]))


if __name__ == "__main__":
    main(sys.argv[1])
