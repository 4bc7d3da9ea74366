"""Turn the FETCH_SIZE / WRITE_SIZE rocprofv3 passes (tools/pmc_run.sh) into profiles/<name>.json (developer tool).

Counters are averaged per launch and corrected as MI355X_MICROARCH.md prescribes for gfx950: FETCH_SIZE (KB) reports
half of the bytes of a wide coalesced streaming read -> doubled; WRITE_SIZE (KB) is exact.
usage: pmc_to_json.py <fetch_dir> <write_dir> <frames_per_launch> <out.json>"""
import csv
import glob
import json
import sys
from collections import defaultdict


def per_kernel(d, counter):
    acc, cnt = defaultdict(float), defaultdict(int)
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter:
                continue
            k = r["Kernel_Name"]
            acc[k] += float(r["Counter_Value"])
            cnt[k] += 1
    return {k: acc[k] / cnt[k] for k in acc}


def main():
    fetch_dir, write_dir, frames, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    fe, wr = per_kernel(fetch_dir, "FETCH_SIZE"), per_kernel(write_dir, "WRITE_SIZE")
    n = 2048
    alg = {"k_col": (4 * n * n + 4 * n * n + 8 * (n // 2 + 2) * (n // 2)) * frames, "k_row_r2c": 8 * n * n * frames,
           "k_row_c2r": (4 * (n // 2 + 2) * n + 4 * n * n) * frames}
    res = {}
    # the column pass of 2048-row frames is k_col<1024, 0, 1, 1, 1> on the "ysplit" route, k_col<2048, 0, ...> otherwise
    for tag, match in (("k_col", ("k_col<1024, 0, 1, 1, 1>", "k_col<2048, 0")), ("k_row_r2c", ("k_row_r2c<2048",)),
                       ("k_row_c2r", ("k_row_c2r<2048, 2, 0",))):
        f = [v for k, v in fe.items() if any(m in k for m in match)]
        w = [v for k, v in wr.items() if any(m in k for m in match)]
        if not f or not w:
            continue
        res[tag] = {"FETCH_SIZE_KB_raw": f[0], "WRITE_SIZE_KB": w[0], "hbm_bytes_per_launch": (2 * f[0] + w[0]) * 1024,
                    "algorithmic_bytes_per_launch": alg[tag], "traffic_over_algorithmic": (2 * f[0] + w[0]) * 1024 / alg[tag]}
    res["hbm_bytes_per_launch"] = res.get("k_col", {}).get("hbm_bytes_per_launch")
    res["frames_per_launch"] = frames
    res["note"] = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes over `bench.py --frames %d --steps 2` (one launch = %d "
                   "frames of 2048x2048); FETCH_SIZE doubled (gfx950 reports 1/2 of streamed read bytes, MI355X_MICROARCH.md)." % (frames, frames))
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
