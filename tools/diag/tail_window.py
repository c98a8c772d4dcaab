#!/usr/bin/env python3
"""The end of one steady-state step, kernel by kernel over BOTH queues: from the end of the second gemm_tn_dma2_kernel (the LSTM
weight gradients at the head of the side queue) to the start of adam_kernel, then the launches and the busy time per kernel
name inside that window.  usage: tail_window.py <r_kernel_trace.csv> [step counted from the last, default 1]"""
import collections, csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
back = int(sys.argv[2]) if len(sys.argv) > 2 else 1
adam = [i for i, r in enumerate(rows) if 'adam_kernel' in r['Kernel_Name']]
hi, lo = adam[-back], adam[-back - 1]
dma2 = [i for i in range(lo, hi) if 'gemm_tn_dma2_kernel' in rows[i]['Kernel_Name']]
t0, t1 = int(rows[dma2[1]]['End_Timestamp']), int(rows[hi]['Start_Timestamp'])
name = lambda r: r['Kernel_Name'].replace('void ', '').replace('(anonymous namespace)::', '')[:58]
win = [r for r in rows[dma2[1] + 1:hi] if int(r['Start_Timestamp']) >= t0]
print(f"--- end of the second gemm_tn_dma2_kernel -> start of adam_kernel: {(t1 - t0) / 1e3:.1f} us wall, {len(win)} kernels, "
      f"{hi - lo} launches in the whole step")
for r in win:
    s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
    print(f"  q{r['Queue_Id']} @{(s - t0) / 1e3:7.1f}  {(e - s) / 1e3:7.1f} us  {name(r)}")
tot = collections.defaultdict(lambda: [0, 0])
for r in win:
    k = r['Kernel_Name'].replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0]
    tot[k][0] += 1
    tot[k][1] += int(r['End_Timestamp']) - int(r['Start_Timestamp'])
print("--- per kernel name inside the window")
for k, (n, t) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
    print(f"  {n:4d} x  {t / 1e3:8.1f} us  {k[:70]}")
