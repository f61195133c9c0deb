"""Per-window figures of the LAST bench step of a rocprofv3 kernel trace (`rocprofv3 --kernel-trace --output-format csv --
python bench.py --gpus 1 --steps 1 --warmup 1`): what the snapshot-scan chain of every window took kernel by kernel, the span from
its first kernel's start to the start of k_decide round 0 (what the scan's time stamps bracket), and the idle gaps in front of
k_decide and of the window's first kernel; then the sums over the step beside the scan_ms the same run reported.
usage: scan_stamp_trace.py <kernel_trace.csv> [<the run's detail file>]"""
import json
import re
import sys

import numpy as np
import pandas as pd

df = pd.read_csv(sys.argv[1]).sort_values("Start_Timestamp").reset_index(drop=True)
df["name"] = df["Kernel_Name"].str.replace(r"^void ", "", regex=True)


def short(n):
    m = re.match(r"_Z(\d+)", n)
    if m:
        k = int(m.group(1))
        return n[m.end():m.end() + k]
    return re.sub(r"[<(].*", "", n)


df["k"] = df["name"].map(short)
df = df[~df["k"].str.startswith("__amd")].reset_index(drop=True)
eps = df.index[df["k"] == "k_eps_neighbours"].tolist()
start = eps[-2] + 1 if len(eps) >= 2 else 0
st = df.iloc[start:eps[-1]].reset_index(drop=True)
CHAIN = {"k_scan_u", "k_scan", "k_pad_rows", "k_prefix16", "k_seed", "k_seed16", "k_seed_merge", "k_scan_a", "k_scan_p", "k_scan_p2",
         "k_scan_p3", "k_missed", "k_pstat_zero"}
cb = st.index[st["k"] == "k_commit_b"].tolist()
rows = []
prev_end = None
lo = 0
for w, e in enumerate(cb):
    win = st.iloc[lo:e + 1]
    # the window starts at its first chain kernel (the first window of a step has the previous step's tail in front)
    ch = win[win["k"].isin(CHAIN)]
    dec = win[win["k"] == "k_decide"]
    if len(ch) == 0 or len(dec) == 0:
        lo = e + 1
        prev_end = st.loc[e, "End_Timestamp"]
        continue
    d0 = dec.iloc[0]
    ch = ch[ch["Start_Timestamp"] < d0["Start_Timestamp"]]
    first = ch.iloc[0]
    win = win[win["Start_Timestamp"] >= first["Start_Timestamp"]]
    kern = (win["End_Timestamp"] - win["Start_Timestamp"]).sum() / 1e3
    end = st.loc[e, "End_Timestamp"]
    rows.append(dict(w=w, chain_us=(ch["End_Timestamp"] - ch["Start_Timestamp"]).sum() / 1e3,
                     dec_minus_first_us=(d0["Start_Timestamp"] - first["Start_Timestamp"]) / 1e3,
                     gap_chain_decide=(d0["Start_Timestamp"] - ch["End_Timestamp"].max()) / 1e3,
                     gap_commit_scan=(first["Start_Timestamp"] - prev_end) / 1e3 if prev_end is not None else np.nan,
                     took=(end - (prev_end if prev_end is not None else first["Start_Timestamp"])) / 1e3, kernels=kern,
                     took_in=(end - first["Start_Timestamp"]) / 1e3, n_queues=win["Queue_Id"].nunique(), first=first["k"]))
    prev_end = end
    lo = e + 1
r = pd.DataFrame(rows)
pd.set_option("display.width", 250)
pd.set_option("display.max_rows", 200)
print(r.round(1).to_string())
print()
print("windows %d  sum chain kernels %.3f ms  sum (k_decide start - first chain kernel start) %.3f ms" % (
    len(r), r["chain_us"].sum() / 1e3, r["dec_minus_first_us"].sum() / 1e3))
print("gap chain end -> k_decide round 0 start: median %.2f us, max %.2f us" % (r["gap_chain_decide"].median(), r["gap_chain_decide"].max()))
g = r["gap_commit_scan"].dropna()
print("gap k_commit_b end -> first chain kernel start: median %.2f us (inside batches: lower quartile %.2f, upper %.2f), max %.2f" % (
    g.median(), g.quantile(0.25), g.quantile(0.75), g.max()))
print("took - kernels, from the window's first chain kernel to its k_commit_b end: median %.2f us  mean %.2f us" % (
    (r["took_in"] - r["kernels"]).median(), (r["took_in"] - r["kernels"]).mean()))
print("took (previous k_commit_b end -> this one) - kernels: median %.2f us" % ((r["took"] - r["kernels"]).median()))
if len(sys.argv) > 2:
    d = json.load(open(sys.argv[2]))
    rf = d.get("roofline") or {}
    print("bench of this trace: ms_per_step %.4f  scan launches %s  scan_ms per step %.4f" % (
        d["ms_per_step"], rf.get("launches"), rf.get("launches", 0) * rf.get("avg_launch_us", 0.0) / 1e3 / d["steps"]))
