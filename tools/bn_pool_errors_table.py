"""profiles/bn_pool_errors.txt from the JSONL that tests/test_bn_pool_kernels_gpu.py appends to the file named by MVF_BN_POOL_ERRORS (one line per reduced
quantity that is compared with the fp64 reference, in the parent process and in every forced leg's child):

    MVF_BN_POOL_ERRORS=/tmp/bn_pool_errors.jsonl python -m pytest -m gpu tests/test_bn_pool_kernels_gpu.py
    python tools/bn_pool_errors_table.py /tmp/bn_pool_errors.jsonl > profiles/bn_pool_errors.txt

The last table is the BOUNDS dictionary of the test module: 4 x the largest measured value per quantity and storage type, capped at 5e-5.
"""
import collections
import json
import sys

CAP = 5e-5
FLOOR = 4 * 2.0 ** -24          # every result is an fp32 number: its own rounding is 2^-24 of it, however exact the sums before it were


def norm(r):
    """The figure a bound is asserted on: the larger of rel_err and rel_l2 outside the slack of the channels that hold undecided mask elements, over the
    conditioning factor."""
    return max(r["net_err"], r["net_l2"]) / r["factor"]


def main(path):
    rows = [json.loads(line) for line in open(path)]
    print("BatchNorm / max-pool training kernels against the fp64 reference: measured error of every reduced quantity")
    print("=" * 110)
    print("tests/test_bn_pool_kernels_gpu.py on an MI355X: every case under the default launch policy and again in one child process per forced policy.")
    print("Reference: tests/bn_pool_ref.py on the operands as stored.  rel_err = helpers.rel_err (max |got - ref| / max |ref|), rel_l2 = helpers.rel_l2.")
    print("factor = the conditioning factor 1 + (mean - K)^2 / (var + eps) of the statistics case whose bound scales by it (else 1); slack ch. = the channels that")
    print("hold undecided mask elements and are granted those elements' |g| (net = the error outside that slack).  Asserted: net <= bound x factor, bound = min(4 x the")
    print("largest net / factor measured over all cases of the quantity and storage type, 5e-5), and never below 4 x 2^-24: the")
    print("results are fp32 numbers, and their own rounding is 2^-24 of them however exact the sums before it were (bf16 pool sums of these sizes ARE exact).")
    print("")
    groups = collections.OrderedDict()
    for r in rows:
        groups.setdefault((r["quantity"], r["dtype"]), []).append(r)
    print("1. Per quantity and storage type (%d measurements)" % len(rows))
    print("")
    print("%-22s %-5s %6s %11s %11s %11s  %s" % ("quantity", "type", "cases", "max norm.", "4 x max", "bound", "worst case (rel_err, rel_l2, factor, policy)"))
    bounds = collections.OrderedDict()
    for key, g in groups.items():
        w = max(g, key=norm)
        b = min(max(4 * norm(w), FLOOR), CAP)
        bounds[key] = b
        print("%-22s %-5s %6d %11.3g %11.3g %11.3g  %s (%.3g, %.3g, %.3g, %s)" % (key + (len(g), norm(w), 4 * norm(w), b, w["case"], w["rel_err"], w["rel_l2"], w["factor"],
                                                                                 w["policy"] or "default")))
    print("")
    print("2. Forced policies: worst case per policy, quantity and storage type")
    print("")
    print("%-18s %-22s %-5s %6s %10s %10s  %s" % ("policy", "quantity", "type", "cases", "rel_err", "rel_l2", "worst case"))
    forced = collections.OrderedDict()
    for r in rows:
        if r["policy"]:
            forced.setdefault((r["policy"], r["quantity"], r["dtype"]), []).append(r)
    for key, g in forced.items():
        w = max(g, key=norm)
        print("%-18s %-22s %-5s %6d %10.3g %10.3g  %s" % (key + (len(g), w["rel_err"], w["rel_l2"], w["case"])))
    print("")
    print("3. Every case under the default policy (a case that is measured more than once -- with and without gm_out / a materialised ga, and with g contiguous or")
    print("   a slice of a tensor 8 / 4 columns wider, the same data -- shows once where the figures are identical, with the number of measurements)")
    print("")
    print("%-46s %-22s %-5s %3s %10s %10s %10s %9s" % ("case", "quantity", "type", "n", "rel_err", "rel_l2", "factor", "slack ch."))
    cases = collections.OrderedDict()
    for r in rows:
        if not r["policy"]:
            name = r["case"]
            for suf in ("_contig", "_c+8", "_c+4"):
                if name.endswith(suf):
                    name = name[:-len(suf)]
            cases.setdefault((name, r["quantity"], r["dtype"], r["rel_err"], r["rel_l2"], r["factor"], r["slack_channels"]), []).append(r)
    for k, g in cases.items():
        print("%-46s %-22s %-5s %3d %10.3g %10.3g %10.3g %9d" % (k[:3] + (len(g),) + k[3:]))
    print("")
    print("4. BOUNDS of tests/test_bn_pool_kernels_gpu.py")
    print("")
    for (q, dt), b in bounds.items():
        print('    ("%s", "%s"): %.2e,' % (q, dt, b))


if __name__ == "__main__":
    main(sys.argv[1])
