"""profiles/stencil_errors.txt from the JSONL that tests/test_stencil_variants_gpu.py appends to the file named by MVF_STENCIL_ERRORS (one line per quantity
that is compared with the fp64 reference, in the parent process and in every forced leg's child):

    MVF_STENCIL_ERRORS=/tmp/stencil_errors.jsonl python -m pytest -m gpu tests/test_stencil_variants_gpu.py
    python tools/stencil_errors_table.py /tmp/stencil_errors.jsonl > profiles/stencil_errors.txt
"""
import collections
import json
import sys

BOUNDS = {
    "y": "32 * 2^-24 * A (+ 2^-8 |ref| in bf16)",
    "stats_sum": "T * pixels_per_wg * 2^-24 * sum |y - K|", "stats_sumsq": "T * pixels_per_wg * 2^-24 * sum (y - K)^2",
    "colsums_sum": "T * pixels_per_wg * 2^-24 * sum |gm|", "colsums_sumsq": "T * pixels_per_wg * 2^-24 * sum gm^2",
    "dw_t": "L * 2^-24 * sum |dy| |x|", "dw_h": "L * 2^-24 * sum |dy| |x|", "dw_w": "L * 2^-24 * sum |dy| |x|",
}


def main(path):
    rows = [json.loads(line) for line in open(path)]
    for r in rows:
        r["leg"] = r["policy"] or "default"
    exact = [r for r in rows if r["cls"] == "int"]
    rnd = [r for r in rows if r["cls"] == "rnd"]
    print("MVF stencil and tap gradients against the fp64 reference: measured error of every case as a fraction of its bound")
    print("=" * 125)
    print("tests/test_stencil_variants_gpu.py on an MI355X: every in-process case under the default launch policy and the cases of every forced policy's child process.")
    print("Reference: tests/stencil_ref.py on the operands as stored.  A = the reference expression on absolute values; sums are compared with the fp64 sums of the")
    print("values the kernel stored; L (T * pixels_per_wg; the tap gradients: rows_per_blk, times T on the (clip, band) kernel) comes from the launch record.")
    print("")
    print("1. Exact class (integer operands): %d comparisons, largest |got - ref| = %g (asserted: 0)" % (len(exact), max([r["max_err"] for r in exact] or [0])))
    print("")
    print("2. Bounded class (normal operands): worst fraction of the bound per policy x kernel x storage type x quantity (%d comparisons)" % len(rnd))
    print("")
    print("%-36s %-8s %-5s %-14s %5s %10s %10s  %-34s %s" % ("policy", "kernel", "type", "quantity", "cases", "max ratio", "max |err|", "worst case", "bound"))
    groups = collections.OrderedDict()
    for r in rnd:
        groups.setdefault((r["leg"], r["kernel"], r["dtype"], r["what"]), []).append(r)
    near = []
    for key, g in groups.items():
        w = max(g, key=lambda r: r["ratio"])
        print("%-36s %-8s %-5s %-14s %5d %10.3g %10.3g  %-34s %s" % (key + (len(g), w["ratio"], max(r["max_err"] for r in g), "%s/%s" % (w["case"], w["variant"]),
                                                                       BOUNDS.get(key[3], ""))))
        if w["ratio"] > 0.5:
            near.append((key, w))
    print("")
    if near:
        print("Within a factor 2 of the bound:")
        for key, w in near:
            print("  %s %s %s %s: %.3g of the bound (%s/%s)" % (key + (w["ratio"], w["case"], w["variant"])))
        if all(key[2] == "bf16" and key[3] == "y" for key, _ in near):
            print("All of these are the bf16 output bound, and they are there by construction: its first term, 2^-8 |ref|, is half an ulp of the stored value when ref is just")
            print("above a power of two, and a correctly rounded result reaches it (ratio -> 1) among a few thousand elements.  The arithmetic error proper is what the fp32")
            print("rows of the same kernels show (at most %.2g of 32 * 2^-24 * A); the bound is not loosened." % max(r["ratio"] for r in rnd if r["dtype"] == "f32" and r["what"] == "y"))
    else:
        print("No measured value comes within a factor 2 of its bound.")


if __name__ == "__main__":
    main(sys.argv[1])
