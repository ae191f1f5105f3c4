"""profiles/pw_bwd_errors.txt from the JSONL that tests/test_pw_bwd_kernels_gpu.py appends to the file named by MVF_PW_BWD_ERRORS (one line per quantity that is
compared with the fp64 reference, in the parent process and in both forced legs' children):

    MVF_PW_BWD_ERRORS=/tmp/pw_bwd_errors.jsonl python -m pytest -m gpu tests/test_pw_bwd_kernels_gpu.py
    python tools/pw_bwd_errors_table.py /tmp/pw_bwd_errors.jsonl > profiles/pw_bwd_errors.txt

The last table is the BOUNDS dictionary of the test module: 4 x the largest measured figure per (kernel, quantity), never above the bound of the existing test
of that quantity and never below 4 x 2^-24.
"""
import collections
import json
import sys

FLOOR = 4 * 2.0 ** -24
# the existing tests' bounds (tests/pw_bwd_cases.py CAPS)
CAPS = {"fused": 2e-5, "pair_s1": 3e-6, "pair_s2": 2e-5, "pw_sums": 2e-6, "pair_wgrad": 5e-5}


def net(r):
    """The figure a bound is asserted on: the larger of the max-norm and 2-norm error outside the allowance."""
    return max(r.get("net_err", 0.0), r.get("net_l2", 0.0))


def quantity_class(q):
    return "slabs" if q.startswith("slabs") else q


def main(path):
    rows = [json.loads(line) for line in open(path)]
    print("Fused pointwise-conv backward kernels against the fp64 reference: measured errors and allowances")
    print("=" * 110)
    print("tests/test_pw_bwd_kernels_gpu.py on an MI355X: every case under the default launch plans and again in one child process per forced plan")
    print("(pwbf_wgs = bnwg_wgs = 1 and = 2).  Reference: tests/pw_bwd_ref.py on the operands as stored.  rel_err = max |got - ref| / max |ref|, rel_l2 the same in")
    print("the 2-norm; allow = the largest allowance of the undecided roundings (from the reference alone) as a share of max |ref|; net = the error outside the")
    print("allowance.  Asserted: net <= bound.  Derived bounds: dx 6e-3 (max-norm), slabs and dw 2e-6 (both norms), dz elementwise (worst |got - ref| over its")
    print("bound 2^-8 |ref| + 8 * 2^-24 A is printed, <= 1).  Measured bounds: 4 x the largest net figure over all cases and legs, within [4 * 2^-24, cap].")
    print("")
    measured = collections.OrderedDict()
    derived = collections.OrderedDict()
    for r in rows:
        if "bound_key" in r:
            measured.setdefault((r["kernel"], r["bound_key"], r["cap"]), []).append(r)
        else:
            derived.setdefault((r["kernel"], quantity_class(r["quantity"])), []).append(r)
    print("1. Quantities with a measured bound (%d measurements)" % sum(len(g) for g in measured.values()))
    print("")
    print("%-11s %-16s %6s %10s %10s %10s %10s %10s  %s" % ("kernel", "quantity", "cases", "max net", "4 x max", "cap", "bound", "max allow", "worst case (rel_err, rel_l2, policy)"))
    bounds = collections.OrderedDict()
    for (kernel, bq, cap), g in measured.items():
        w = max(g, key=net)
        b = min(max(4 * net(w), FLOOR), CAPS[cap])
        bounds[(kernel, bq)] = b
        print("%-11s %-16s %6d %10.3g %10.3g %10.3g %10.3g %10.3g  %s (%.3g, %.3g, %s)" % (kernel, bq, len(g), net(w), 4 * net(w), CAPS[cap], b, max(r["allow"] for r in g), w["case"],
                                                                                       w["rel_err"], w["rel_l2"], w["policy"] or "default"))
    print("")
    print("2. Quantities with a derived bound (%d measurements)" % sum(len(g) for g in derived.values()))
    print("")
    print("%-13s %-10s %6s %10s %10s %10s %10s  %s" % ("kernel", "quantity", "cases", "max net", "bound", "max rel", "max allow", "worst case (policy)"))
    for (kernel, q), g in derived.items():
        if "worst_over_bound" in g[0]:
            w = max(g, key=lambda r: r["worst_over_bound"])
            print("%-13s %-10s %6d %10.3g %10.3g %10s %10s  %s (%s)" % (kernel, q, len(g), w["worst_over_bound"], 1.0, "-", "-", w["case"], w["policy"] or "default"))
        else:
            w = max(g, key=net)
            print("%-13s %-10s %6d %10.3g %10.3g %10.3g %10.3g  %s (%s)" % (kernel, q, len(g), net(w) if q != "dx" else w["net_err"], w["bound"], max(r["rel_err"] for r in g),
                                                                        max(r["allow"] for r in g), w["case"], w["policy"] or "default"))
    print("")
    print("3. Forced plans: worst figure per plan, kernel and quantity")
    print("")
    print("%-26s %-11s %-16s %6s %10s %10s  %s" % ("policy", "kernel", "quantity", "cases", "max net", "max allow", "worst case"))
    forced = collections.OrderedDict()
    for r in rows:
        if r["policy"] and "worst_over_bound" not in r:
            forced.setdefault((r["policy"], r["kernel"], r.get("bound_key", quantity_class(r["quantity"]))), []).append(r)
    for key, g in forced.items():
        w = max(g, key=net)
        print("%-26s %-11s %-16s %6d %10.3g %10.3g  %s" % (key + (len(g), net(w), max(r["allow"] for r in g), w["case"])))
    print("")
    print("4. Every case under the default plans: the largest figures over the case's quantities")
    print("")
    print("%-13s %-44s %3s %10s %10s %10s" % ("kernel", "case", "n", "max rel", "max net", "max allow"))
    cases = collections.OrderedDict()
    for r in rows:
        if not r["policy"] and "worst_over_bound" not in r and r.get("quantity") != "dx":
            cases.setdefault((r["kernel"], r["case"]), []).append(r)
    for (kernel, case), g in cases.items():
        print("%-13s %-44s %3d %10.3g %10.3g %10.3g" % (kernel, case, len(g), max(r["rel_err"] for r in g), max(net(r) for r in g), max(r["allow"] for r in g)))
    print("")
    print("5. BOUNDS of tests/test_pw_bwd_kernels_gpu.py")
    print("")
    for (kernel, bq), b in bounds.items():
        print('    ("%s", "%s"): %.2e,' % (kernel, bq, b))


if __name__ == "__main__":
    main(sys.argv[1])
