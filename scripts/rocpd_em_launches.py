"""Durations of the em_batch_kernel launches of a traced bench run from a rocprofv3 rocpd database (dev tool): the sliced
launches' median / range and the last launch (the flush, where the slowest image finishes alone).
   python scripts/rocpd_em_launches.py t.db"""
import sqlite3
import sys

import numpy as np


def main(db):
    cur = sqlite3.connect(db).cursor()
    tables = [r[0] for r in cur.execute("select name from sqlite_master where type in ('table','view')")]
    disp = [t for t in tables if t.startswith("rocpd_kernel_dispatch")][0]
    sym = [t for t in tables if t.startswith("rocpd_info_kernel_symbol")][0]
    scols = [r[1] for r in cur.execute("pragma table_info(%s)" % sym)]
    name_col = "kernel_name" if "kernel_name" in scols else "display_name"
    rows = list(cur.execute("select d.start, d.end, s.%s from %s d join %s s on d.kernel_id = s.id order by d.start" % (name_col, disp, sym)))
    em = np.array([(en - st) / 1e6 for st, en, name in rows if "em_batch_kernel" in name])
    if em.size < 2:
        print("no EM launches")
        return
    sliced = em[:-1]
    print("em_batch_kernel launches: %d" % em.size)
    print("sliced launches (ms): median %.3f, min %.3f, max %.3f, sum %.2f" % (np.median(sliced), sliced.min(), sliced.max(), sliced.sum()))
    print("last %d sliced launches (ms): %s" % (min(8, sliced.size), " ".join("%.3f" % v for v in sliced[-8:])))
    print("last launch, the flush (ms): %.3f" % em[-1])


if __name__ == "__main__":
    main(sys.argv[1])
