"""Model of k_dsmp's step classes: wave-instructions (VALU) per signature of one
wave's pool under the step rules of fd_ed25519_pool.h, for the variants

  today      every step pays the frame; a DBL step the DBL body, a mixed step the union body
  add-only   a mixed step whose selection holds no DBL slot runs the ADD-only body
  dbl-nopop  a DBL step skips the event-pop path
  pair       when at least 64 slots have two doublings ahead, one step runs both
  all        the three together

Op streams come from the ref10 slide of random scalars (as tools/r04_pool_assign_model.py);
selection is in slot order, without the kernel's longest-first drain.  The step costs are
arguments: take them from tools/isa_pool.sh.  The defaults are the counts of the build
before the classes were split (frame 71, DBL body 969, mixed body 1397 VALU) and the
savings estimated then.  This is a model of instruction counts, not a measurement.

usage: python tools/pool_model.py [--pool 112] [--sigs 512] [--frame 71] [--dbl 969] [--mixed 1397]
                                  [--add-only-saving 110] [--dbl-pop-saving 25] [--seed 1]
"""
import argparse
import random

L = 2**252 + 27742317777372353535851937790883648493


def slide(a):
    r = [(a >> i) & 1 for i in range(256)]
    for i in range(256):
        if r[i]:
            for b in range(1, 7):
                if i + b >= 256:
                    break
                if r[i + b]:
                    if r[i] + (r[i + b] << b) <= 15:
                        r[i] += r[i + b] << b
                        r[i + b] = 0
                    elif r[i] - (r[i + b] << b) >= -15:
                        r[i] -= r[i + b] << b
                        for k in range(i + b, 256):
                            if not r[k]:
                                r[k] = 1
                                break
                            r[k] = 0
                    else:
                        break
    return r


def ops(h, s):
    """0 = DBL, 1 = ADD-A, 2 = ADD-B, from the top digit down."""
    a, b = slide(h), slide(s)
    top = max([i for i in range(256) if a[i] or b[i]] or [0])
    o = []
    for i in range(top, -1, -1):
        o.append(0)
        if a[i]:
            o.append(1)
        if b[i]:
            o.append(2)
    return o


def sim(streams, P, c, add_only, dbl_nopop, pair):
    q = list(range(len(streams)))
    cur, pos = [None] * P, [0] * P
    valu = steps = lanes = n_pair = n_addonly = 0
    while True:
        for sl in range(P):
            if cur[sl] is None and q:
                cur[sl], pos[sl] = q.pop(), 0
        live = [sl for sl in range(P) if cur[sl] is not None]
        if not live:
            break
        st = {sl: streams[cur[sl]] for sl in live}
        D = [sl for sl in live if st[sl][pos[sl]] == 0]
        A = [sl for sl in live if st[sl][pos[sl]] != 0]
        two = [sl for sl in D if pos[sl] + 1 < len(st[sl]) and st[sl][pos[sl] + 1] == 0]
        adv = 1
        if pair and q and len(two) >= 64:                     # main phase only
            sel, cost, adv = two[:64], c.frame + 2 * c.dbl - (c.dbl_pop_saving if dbl_nopop else 0), 2
            n_pair += 1
        elif len(D) >= 64 or not A:
            sel, cost = D[:64], c.frame + c.dbl - (c.dbl_pop_saving if dbl_nopop else 0)
        else:
            sel, cost = (A + D)[:64], c.frame + c.mixed
            if add_only and len(A) >= len(sel):
                cost -= c.add_only_saving
                n_addonly += 1
        valu += cost
        steps += 1
        lanes += len(sel)
        for sl in sel:
            pos[sl] += adv
            if pos[sl] == len(st[sl]):
                cur[sl] = None
    return valu / len(streams), steps, lanes / (64.0 * steps), n_pair, n_addonly


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=112)
    ap.add_argument("--sigs", type=int, default=512, help="signatures per wave")
    ap.add_argument("--frame", type=int, default=71, help="per-step VALU outside the bodies")
    ap.add_argument("--dbl", type=int, default=969)
    ap.add_argument("--mixed", type=int, default=1397)
    ap.add_argument("--add-only-saving", type=int, default=110)
    ap.add_argument("--dbl-pop-saving", type=int, default=25)
    ap.add_argument("--seed", type=int, default=1)
    c = ap.parse_args()
    random.seed(c.seed)
    streams = [ops(random.getrandbits(512) % L, random.getrandbits(512) % L) for _ in range(c.sigs)]
    runs = sum(1 for s in streams for i in range(len(s)) if s[i] == 0 and
               ((i and s[i - 1] == 0) or (i + 1 < len(s) and s[i + 1] == 0)))
    print("P %d, %d signatures per wave, %.1f ops per signature, %.1f %% of doublings in runs of two or more"
          % (c.pool, c.sigs, sum(map(len, streams)) / c.sigs, 100.0 * runs / sum(s.count(0) for s in streams)))
    print("| variant | VALU per signature | change | steps | fill | pair steps | ADD-only steps |")
    print("|---|---|---|---|---|---|---|")
    base = None
    for name, a, d, p in (("today", 0, 0, 0), ("add-only", 1, 0, 0), ("dbl-nopop", 0, 1, 0), ("pair", 0, 0, 1),
                          ("all", 1, 1, 1)):
        v, steps, fill, n_pair, n_ao = sim(streams, c.pool, c, a, d, p)
        base = base or v
        print("| %s | %.0f | %+.1f %% | %d | %.3f | %d | %d |" % (name, v, 100.0 * (v / base - 1), steps, fill, n_pair, n_ao))


if __name__ == "__main__":
    main()
