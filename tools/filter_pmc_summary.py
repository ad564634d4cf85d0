"""Adds the rocprofv3 FETCH_SIZE of the masked scan to tools/filter_probe.py's JSON: per row, the bytes one launch
of the masked scan (scan_kernel<QH, 1, Op16<DT>, WalkLive>) read (2 * FETCH_SIZE * 1024: gfx950 counts 64 B per 128-B request of a wide streaming read,
as in tools/summarize_profile.py) against the bytes of the live row blocks.

    python tools/filter_pmc_summary.py PROBE_JSON PMC_DIR_OF_ROW:ROW [...] --out OUT_JSON
(PMC_DIR: the -d directory of `rocprofv3 --pmc FETCH_SIZE -- python tools/filter_probe.py --only ROW`)"""
import argparse
import csv
import glob
import json
import os


def scan_fetch_bytes(pmc_dir):
    """Median over the launches of the masked scan of 2 * FETCH_SIZE * 1024, and the launch count."""
    vals = {}
    for f in glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if r["Counter_Name"] != "FETCH_SIZE" or not ("scan_kernel" in r["Kernel_Name"] and "Op16" in r["Kernel_Name"] and "WalkLive" in r["Kernel_Name"]):
                    continue
                key = (f, r.get("Dispatch_Id") or r.get("Correlation_Id"))
                vals[key] = vals.get(key, 0.0) + float(r["Counter_Value"])
    v = sorted(vals.values())
    if not v:
        return None, 0
    return 2 * v[len(v) // 2] * 1024, len(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("probe")
    ap.add_argument("pmc", nargs="+", help="DIR:ROW")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    out = json.load(open(a.probe))
    for spec in a.pmc:
        d, row = spec.rsplit(":", 1)
        b, n = scan_fetch_bytes(d)
        rec = out["rows"].setdefault(row, {})
        rec["pmc_scan_fetch_bytes"] = None if b is None else int(b)
        rec["pmc_scan_launches"] = n
        if b is not None and rec.get("live_bytes"):
            rec["pmc_fetch_over_live_bytes"] = round(b / rec["live_bytes"], 4)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["rows"], indent=1))


if __name__ == "__main__":
    main()
