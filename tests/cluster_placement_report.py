"""Developer tool beside cluster_rows_timeline.py and cluster_spill_report.py (same arguments: scene, settle steps; same trace,
mi_debug_flow_trace): which CLASS of task the iteration's chain passes through, and what the closing colours of the large first tasks
look like.  A task's class is where its rows live (k_cluster_solve.hip: registers at the closing end, LDS, the global scratch at the
opening end): register-run (slot 0, all rows in registers), mixed (slot 0, rows beyond the registers), LDS-run (slots >= 1) without or
with scratch rows.  Per phase: the classes' tasks, colour loops (median, slowest) and the slowest task of the phase with its class.  For
the mixed first tasks: from the colour sizes of iteration 10 (trace rows 7-8), the closing colours that fall into the last 16 positions
and into the last block of 16 counted from regBase (what the one-wave tail can run), and the colours the tail did run (row 15, words 27..).
(cluster_spill_report.py's header still describes the sweep it was written for, in which one scratch row sent all of a task's colours outside
the registers through the general row step; its figures are right as they are, but since the scratch takes a task's OPENING positions only
the colours that begin below them run that step.)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import directx_renderer_kurth_amd as mi
from directx_renderer_kurth_amd import scenes
name = sys.argv[1]; settle = int(sys.argv[2])
s = scenes.by_name(name)
w = s.instantiate(mi.World())
for i in range(settle + 5):
    w.step_internal(s.dt)
w.synchronize()
st = w.stats()
print({k: st[k] for k in ("numCollisions", "numContacts", "numColors", "clusterTasks", "clusterManifolds", "numFlowRecoveries")})
w.flow_trace(True)
w.step_internal(s.dt); w.synchronize()
G = 256
raw = w.flow_trace(True, G * 16).astype(np.int64).reshape(G, 16, 32)
t0 = raw[raw[:, 15, 1] > 0, 15, 0].min()
us = lambda x: (x - t0) * 0.01
iters = 30
classes = ("register-run", "mixed", "LDS-run", "LDS-run with scratch rows")
rec = []                                                             # (phase, class, loop us, colours, contacts, slot, workgroup)
for k in range(5):
    hk = np.nonzero(raw[:, 3 * k, 0] > 0)[0]
    if not len(hk): continue
    loop = np.median(us(raw[hk, 3 * k + 1, :iters]) - us(raw[hk, 3 * k, :iters]), axis=1)
    ncol = raw[hk, 15, 3 + 4 * k]; word = raw[hk, 15, 5 + 4 * k]; nct = word >> 32; ph = word & 0xFF
    reg = raw[hk, 15, 22 + k] >> 32; in_lds = raw[hk, 15, 22 + k] & 0xFFFFFFFF
    spilled = nct - reg - in_lds
    cls = np.where(k == 0, np.where(nct > reg, 1, 0), np.where(spilled > 0, 3, 2))
    if k == 0: cls = np.where((reg == 0) & (nct > 0), np.where(spilled > 0, 3, 2), cls)   # (MI_CLUSTER_REG_CONTACTS=0)
    for j in range(len(hk)):
        if ncol[j] > 0: rec.append((int(ph[j]), int(cls[j]), float(loop[j]), int(ncol[j]), int(nct[j]), k, int(hk[j])))
rec = np.array(rec)
for p in np.unique(rec[:, 0]):
    r = rec[rec[:, 0] == p]
    slow = r[r[:, 2].argmax()]
    print("phase %d: %d tasks; slowest colour loop %.2f us: %s, slot %d, %d colours, %d contacts, %.3f us per colour" % (p, len(r), slow[2], classes[int(slow[1])], slow[5], slow[3], slow[4], slow[2] / slow[3]))
    for c in range(4):
        q = r[r[:, 1] == c]
        if len(q): print("    %-26s %3d tasks: colour loop median %.2f slowest %.2f us; per colour median %.3f us; colours mean %.1f max %d" % (classes[c], len(q), np.median(q[:, 2]), q[:, 2].max(), np.median(q[:, 2] / q[:, 3]), q[:, 3].mean(), q[:, 3].max()))
# the mixed first tasks' closing colours
sizes = raw[:, 7:9].reshape(G, -1)[:, :63]
nct0 = raw[:, 15, 5] >> 32; reg0 = raw[:, 15, 22] >> 32; ncol0 = raw[:, 15, 3]; tail0 = raw[:, 15, 27] >> 32
mixed = np.nonzero((raw[:, 0, 0] > 0) & (nct0 > reg0) & (reg0 > 0) & (ncol0 > 0) & (ncol0 <= 63))[0]
last16, block, small = [], [], []
for g in mixed:
    sz = sizes[g, :ncol0[g]]; start = np.concatenate([[0], np.cumsum(sz)[:-1]]); end = int(sz.sum()); base = int(nct0[g] - reg0[g])
    last16.append(int((start >= end - 16).sum()))
    block.append(int(((start >= base) & ((start - base) >> 4 == (end - base - 1) >> 4)).sum()) if end > base else 0)
    small.append(int((sz <= 16).sum()))
if len(mixed):
    print("mixed first tasks (%d): closing colours within the last 16 positions: mean %.1f max %d; within the last block of 16 from regBase: mean %.1f max %d (tasks with two or more: %d); colours of at most 16 rows: mean %.1f; colours the one-wave tail ran: mean %.1f max %d (tasks: %d)"
          % (len(mixed), np.mean(last16), max(last16), np.mean(block), max(block), sum(b >= 2 for b in block), np.mean(small), tail0[mixed].mean(), tail0[mixed].max(), (tail0[mixed] >= 2).sum()))
    slowest = mixed[np.argmax(ncol0[mixed])]
    print("    the mixed task with most colours (%d, %d contacts): colour sizes %s" % (ncol0[slowest], nct0[slowest], sizes[slowest, :ncol0[slowest]].tolist()))
k0 = raw[:, 0, 0] > 0
print("period (slot 0, median over workgroups and iterations): %.2f us" % np.median(np.diff(us(raw[k0, 0, :iters]), axis=1)))
