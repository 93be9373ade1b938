"""Stretch between the last forward conv_pointwise<256,3,false> and the first backward conv_pointwise<128,4,true> around each
detection_loss_bwd_kernel of a rocprofv3 rocpd database: wall, busy (union of kernel intervals), idle, launches; and per-step rows of the
head kernels.  usage: python tools/prof_stretch.py <results.db> <steps>"""
import re, sqlite3, statistics, sys
db, steps = sys.argv[1], float(sys.argv[2])
c = sqlite3.connect(db)
rows = c.execute("select name, start, end from kernels order by start").fetchall()
fwd = re.compile(r"conv_pointwise_kernel<256, ?3, ?false")
bwd = re.compile(r"conv_pointwise_kernel<128, ?4, ?true")
anchors = [i for i, r in enumerate(rows) if "detection_loss_bwd_kernel" in r[0]]
res = []
for a in anchors:
    i = a
    while i >= 0 and not fwd.search(rows[i][0]): i -= 1
    j = a
    while j < len(rows) and not bwd.search(rows[j][0]): j += 1
    if i < 0 or j >= len(rows): continue
    t0, t1 = rows[i][2], rows[j][1]
    seg = [r for r in rows[i + 1:j]]
    busy, cur_s, cur_e = 0, None, None
    for _, s, e in sorted((r for r in seg), key=lambda r: r[1]):
        s, e = max(s, t0), min(e, t1)
        if e <= s: continue
        if cur_e is None or s > cur_e:
            if cur_e is not None: busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else: cur_e = max(cur_e, e)
    if cur_e is not None: busy += cur_e - cur_s
    res.append(((t1 - t0) / 1e3, busy / 1e3, (t1 - t0 - busy) / 1e3, len(seg)))
print("stretches found %d" % len(res))
for r in res: print("  wall %8.1f us  busy %8.1f us  idle %8.1f us  launches %d" % r)
if res:
    print("median wall %.1f us  busy %.1f us  idle %.1f us  launches %d" % tuple(statistics.median(x[k] for x in res) for k in range(4)))
print("total launches/step %.1f" % (len(rows) / steps))
pat = re.compile(r"head_split|heads_split|heads_grad_pad|cast_pad_kernel|fill|Fill|vectorized_elementwise")
agg = {}
for n, s, e in rows:
    if pat.search(n):
        k = n[:110]
        a_ = agg.setdefault(k, [0, 0]); a_[0] += 1; a_[1] += e - s
for k, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    print("%-110s %6.1f /step %8.2f us/step %6.2f us avg" % (k, n / steps, t / 1e3 / steps, t / 1e3 / n))
