"""Digest of what tests/test_rnea_backward_param_rungs.py prints, as committed in profiles/rnea_backward_param_rungs_tests.txt:

    cd tests
    pytest test_rnea_backward_param_rungs.py -m "not gpu" -s > host.txt        # any box
    pytest test_rnea_backward_param_rungs.py -m gpu -s > gpu.txt               # an MI355X
    python ../tools/digest_param_rungs.py host.txt gpu.txt > ../profiles/rnea_backward_param_rungs_tests.txt

The module prints one RNEAPRUNG line per link, group and comparison (47 000 lines); the digest keeps, per run,
  * the worst ratio err / max(yardstick, floor) per path or rung and group, over the RNEAPRUNG-WORST lines (one per launch; the batch
    size, "-abi" and "+tail" are taken out of the path's name, the mutations' comparisons left out),
  * per robot, level, link and group the RNEAPRUNG-EXCEPTED lines (worst ratio against the issue's floor, and with the product scale) and
    the RNEAPRUNG-FLOOR ... DECIDES lines (worst ratio without any floor, widest floor),
  * the number of RNEAPRUNG-FLOORGRP lines per robot,
  * verbatim, once each: RNEAPRUNG-TRUTH, RNEAPRUNG-MUTATION, RNEAPRUNG-NOTE, and the RNEABRUNG-BITS lines that tell rungs apart (the
    partial sums of the `single` path, the refused fan, arm-param-own against the library's kernel, the misaligned pointer)."""
import collections
import re
import sys


def lines_of(path):
    out, seen = [], set()
    for line in open(path).read().split("\n"):
        line = line.lstrip(".FEsx")           # (pytest's progress marks in front of a printed line)
        if line.startswith("RNEA") and line not in seen:
            seen.add(line)
            out.append(line)
    return out


def family(path):
    return re.sub(r"\[.*\]", "", re.sub(r"-B\d+", "", path).replace("-abi", "").replace("+tail", ""))


def worst(lines):
    w, n = collections.defaultdict(lambda: collections.defaultdict(float)), collections.Counter()
    for line in lines:
        if not line.startswith("RNEAPRUNG-WORST"):
            continue
        tok = line.split()
        p = family(tok[2])
        if p.startswith("mutation"):
            continue
        n[p] += 1
        for k in range(tok.index("N") + 2, len(tok) - 1, 2):
            w[p][tok[k]] = max(w[p][tok[k]], float(tok[k + 1]))
    return ["  %-34s %5d launches   %s" % (p, n[p], "  ".join("%s %.2f" % kv for kv in w[p].items())) for p in sorted(w)]


def per_group(lines, tag, fields):
    """fields(tokens, index of "link") -> the floats to take the largest of"""
    d = {}
    for line in lines:
        if not line.startswith(tag):
            continue
        t = line.split()
        i = t.index("link")
        if t[2].startswith("mutation"):
            continue
        key = (t[1], "param" if ":param" in t[2] else "op", int(t[i + 1]), t[i + 2], "below 64 rows" if int(t[t.index("N") + 1]) < 64 else "64 rows and more")
        vals = fields(t, i)
        have = d.setdefault(key, [0] + [0.0] * len(vals))
        have[0] += 1
        have[1:] = [max(a, b) for a, b in zip(have[1:], vals)]
    return sorted(d.items())


def digest(name, lines):
    out = ["==== " + name + " ====", "worst err / max(yardstick, floor) per path or rung:"] + worst(lines)
    out.append("EXCEPTED groups (worst ratio against the issue's floor max(yardstick, 2^-23 max(A, rotation scale)); with the product scale):")
    out += ["  %-36s %-5s link %2d %-12s %-16s %4d comparisons   %12.2f   %6.2f" % (k + tuple(v))
            for k, v in per_group(lines, "RNEAPRUNG-EXCEPTED", lambda t, i: (float(t[t.index("with") - 1].rstrip(";")), float(t[-1])))]
    out.append("where the floor DECIDES (worst ratio with no floor at all, against max(yardstick, 2^-23); widest floor in units of 2^-23):")
    out += ["  %-36s %-5s link %2d %-12s %-16s %4d comparisons   %14.2f   %10.3e" % (k + tuple(v))
            for k, v in per_group(lines, "RNEAPRUNG-FLOOR ", lambda t, i: (float(t[-2]), float(t[i + 4])))]
    groups = collections.Counter(line.split()[1] for line in lines if line.startswith("RNEAPRUNG-FLOORGRP"))
    if groups:
        out.append("RNEAPRUNG-FLOORGRP lines (256 rows, two seeds, three cases: the floor exceeds twice max(yardstick, 2^-23)) per robot: "
                   + ", ".join("%s %d" % kv for kv in sorted(groups.items())))
    out += [line for line in lines if line.startswith(("RNEAPRUNG-TRUTH", "RNEAPRUNG-MUTATION", "RNEAPRUNG-NOTE"))]
    bits = [line for line in lines if line.startswith("RNEABRUNG-BITS")]
    out.append("bit comparisons: %d asserted equal or different as stated, of which:" % len(bits))
    return out + [line for line in bits if re.search(r"partial sums|prefix-mask|refused|arm-param-own vs|misaligned", line)] + [""]


if __name__ == "__main__":
    print("tests/test_rnea_backward_param_rungs.py: the digest that tools/digest_param_rungs.py makes of what the module prints (see there)\n")
    print("\n".join(digest("without a GPU: host build, host emulation under g++ and the ROCm clang", lines_of(sys.argv[1]))
                    + digest("MI355X (pytest -m gpu)", lines_of(sys.argv[2]))))
