#!/usr/bin/env python3
"""Summarise a tools/profile_bench.sh run: per-kernel durations (kernel traces, one per workload) and per-kernel counters
(one PMC run per counter set and workload), with the derived figures DESIGN.md uses.  Reads <out>/trace_<w>/,
<out>/pmc_<w>_<i>/ and <out>/cal_<i>/ for the workloads in WORKLOADS (missing ones are reported empty).  The product kernel
of a CG workload is CgFusedEpiT where the passes are fused (template value 11 = storage format 9; 14 / 15 / 16: the
general-geometry march kernels).  Writes spmv_traffic.json (fabric-side bytes per launch of the product kernels, stamped
with the fingerprint of the kernel sources) next to the summary."""
import collections
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_csv(pattern):
    rows = []
    for f in glob.glob(pattern, recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    return rows


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    m = re.match(r"(?:void )?(mk_\w+_kernel<[^(]*>)\(", name)
    if m:
        return m.group(1).replace(" ", "")
    return name.split("(")[0][:60]


def trace(out, sub, title):
    tr = read_csv(os.path.join(out, sub, "**", "*kernel_trace.csv"))
    agg = collections.OrderedDict()
    for r in tr:
        d = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        a = agg.setdefault(short(r["Kernel_Name"]), [0, 0])
        a[0] += 1
        a[1] += d
    tot = sum(a[1] for a in agg.values()) or 1
    print("== %s: kernel trace (calls, avg us, share of GPU time)" % title)
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1][1])[:14]:
        print("%-78s %7d %10.2f %6.2f%%" % (k[:78], a[0], a[1] / a[0] / 1e3, 100.0 * a[1] / tot))
    print()
    return {k: a[1] / a[0] / 1e3 for k, a in agg.items()}


def counters(out, prefix):
    acc = collections.OrderedDict()
    for d in sorted(glob.glob(os.path.join(out, prefix + "_*"))):
        if not os.path.isdir(d):
            continue
        for r in read_csv(os.path.join(d, "**", "*counter_collection.csv")):
            key = (short(r["Kernel_Name"]), r["Counter_Name"])
            a = acc.setdefault(key, [0, 0.0])
            a[0] += 1
            a[1] += float(r["Counter_Value"])
    tab = collections.OrderedDict()
    for (k, c), a in acc.items():
        if a[0] >= 10:
            tab.setdefault(k, {})[c] = a[1] / a[0]
            tab[k]["_n"] = a[0]
    return tab


def report(tab, durations, title, want):
    print("== %s: counters per launch (averages), derived figures" % title)
    for k, c in tab.items():
        if not any(w in k for w in want):
            continue
        print("--", k, "(launches per pass: %d)" % c.get("_n", 0))
        for name in sorted(c):
            if name != "_n":
                print("     %-34s %16.1f" % (name, c[name]))
        g = c.get("GRBM_GUI_ACTIVE")
        if g:
            cyc = g / 8.0                                   # summed over the 8 XCDs
            if "TA_TA_BUSY_sum" in c:
                print("     > texture-address unit busy             %5.1f %% of the kernel (256 CUs)" % (100 * c["TA_TA_BUSY_sum"] / 256 / cyc))
            if "TA_FLAT_READ_WAVEFRONTS_sum" in c:
                print("     > TA busy cycles per wave-level read    %5.1f" % (c["TA_TA_BUSY_sum"] / c["TA_FLAT_READ_WAVEFRONTS_sum"]))
        if "TCC_HIT_sum" in c and "TCC_MISS_sum" in c:
            print("     > L2 hit rate                           %5.1f %%" % (100 * c["TCC_HIT_sum"] / (c["TCC_HIT_sum"] + c["TCC_MISS_sum"])))
        if "TCP_TCC_READ_REQ_sum" in c and "TCP_TOTAL_CACHE_ACCESSES_sum" in c:
            print("     > L1 -> L2 read requests per L1 access   %5.3f" % (c["TCP_TCC_READ_REQ_sum"] / c["TCP_TOTAL_CACHE_ACCESSES_sum"]))
        if "SQ_WAIT_ANY" in c and "SQ_WAVE_CYCLES" in c:
            print("     > waves waiting (s_waitcnt / barrier)    %5.1f %% of wave time; issue stalls %5.1f %%" %
                  (100 * c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"], 100 * c.get("SQ_WAIT_INST_ANY", 0) / c["SQ_WAVE_CYCLES"]))
        if "SQ_LDS_BANK_CONFLICT" in c and "SQ_LDS_IDX_ACTIVE" in c and c["SQ_LDS_IDX_ACTIVE"]:
            print("     > LDS bank-conflict cycles               %5.1f %% of LDS-active cycles" % (100 * c["SQ_LDS_BANK_CONFLICT"] / c["SQ_LDS_IDX_ACTIVE"]))
        if "FETCH_SIZE" in c or "WRITE_SIZE" in c:
            rd, wr = c.get("FETCH_SIZE", 0) * 2048.0, c.get("WRITE_SIZE", 0) * 1024.0
            us = durations.get(k)
            print("     > fabric-side bytes per launch: read %.1f MB (FETCH_SIZE x 2048, calibrated), written %.1f MB (WRITE_SIZE x 1024)%s"
                  % (rd / 1e6, wr / 1e6, "; %.2f TB/s over the traced %.1f us" % ((rd + wr) / us / 1e6, us) if us else ""))
        print()


WORKLOADS = [("varcoef", "poisson3d-512-varcoef@1", "CG, 512^3 variable coefficients (second workload of the line)"),
             ("const", "poisson3d-512@1", "CG, 512^3 constant coefficients (the line's headline: BASELINE configs[4])"),
             ("p500", "poisson3d-500@1", "CG, 500^3 constant coefficients: the general-geometry brick march (round 6)"),
             ("plain", "csr_plain@1", "CG, 512^3 constant coefficients FORCED to plain CSR (storage format 0): north_star's literal kernel"),
             ("p2d", "poisson2d-1000@1", "CG, 2-D n = 1e6"),
             ("others", None, "the nine other solver loops: BiCGSTAB / CGS / TFQMR (random n = 1e6), MINRES / SYMMLQ (shifted 2-D n = 4e6), LSQR / LSMR / CRAIG / CRAIG-MR (random 4e6 x 1e6)")]


def main():
    out = sys.argv[1]
    import bench
    traffic = {"kernel_source_sha": bench.kernel_source_sha(), "measured": os.path.basename(out.rstrip("/")),
               "unit": "bytes per launch at the L2's fabric side: FETCH_SIZE x 2048 + WRITE_SIZE x 1024 (calibrated; "
                       "Infinity-Cache hits are counted)"}
    trace(out, "trace_default", "python bench.py (the driver's command: every workload in one process)")
    for w, key, title in WORKLOADS:
        dur = trace(out, "trace_" + w, title)
        tab = counters(out, "pmc_" + w)
        want = ("CgSpmvEpi", "CgFusedEpi", "CgUpdate", "cg_beta") if key else ("mk_spmv_kernel", "mk_stream_kernel")
        report(tab, dur, title, want)
        for k, c in tab.items():
            if "mk_spmv_kernel" in k and "Partial" not in k and "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                fmt = int(k.rstrip(">").split(",")[-1])
                ent = {"bytes": int(c["FETCH_SIZE"] * 2048 + c["WRITE_SIZE"] * 1024),
                       "read_bytes": int(c["FETCH_SIZE"] * 2048), "written_bytes": int(c["WRITE_SIZE"] * 1024),
                       "format": {6: 5, 11: 9, 12: 10, 13: 11, 14: 9, 15: 10, 16: 11}.get(fmt, fmt), "kernel": k, "avg_us_in_trace": dur.get(k)}
                if key and key.startswith("stencil27"):      # (template values 7 / 8 -> formats 7 / 8)
                    ent["format"] = fmt
                if key and "CgFusedEpi" in k:                 # fused passes: THE product kernel of the workload
                    traffic[key] = ent
                elif key and "CgSpmvEpi" in k and "CgFusedEpi" not in traffic.get(key, {}).get("kernel", ""):
                    traffic[key] = ent
                elif not key:
                    traffic.setdefault("other_configs", {})[k] = ent
    cal = counters(out, "cal")
    print("== calibration (1 GiB streams): counter per launch -> bytes per count")
    for k, c in cal.items():
        for name in ("FETCH_SIZE", "WRITE_SIZE"):
            if name in c and (("read" in k) == (name == "FETCH_SIZE")):
                print("   %-60s %-11s %12.1f -> %.1f B/count" % (k[:60], name, c[name], 1073741824.0 / c[name]))
    json.dump(traffic, open(os.path.join(out, "spmv_traffic.json"), "w"), indent=1)
    print("\n== spmv_traffic.json\n" + json.dumps(traffic, indent=1))


if __name__ == "__main__":
    main()
