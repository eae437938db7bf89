"""The two launch chains of the batched S3 env step from rocprofv3 kernel traces (CSV), one line of figures per trace directory:
   rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/time_rollout.py 128 1 30 2
   python tools/chain_lengths.py DIR [DIR ...]
Per directory: means of `smooth_linear_kernel` and of the flow stream's `topology_kernel` over the second half of their
launches (and the per-launch series, for pairing two traces by launch index: `--series`), and - medians over the chains of the
second half - each chain's kernel sum, the gaps between its kernels and the wait in front of its first kernel.  The main chain
is the queue of `smooth_linear_kernel` from `remesh` to the Q-head, the flow chain the other queue with `topology_kernel` launches, from its
`topology_kernel` to `at_correction_kernel`."""
import csv, glob, statistics, sys


def load(d):
    ev = []
    for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), r["Kernel_Name"].split("(")[0]))
    ev.sort()
    return ev


def queue_of(ev, name):
    q = {}
    for _, _, qu, n in ev:
        if name in n:
            q[qu] = q.get(qu, 0) + 1
    return max(q, key=q.get)


def chains(ev, queue, first, last):
    """Chains of one queue: from a kernel whose name holds `first` to the next whose name holds `last` ->
    list of (kernel sum, gaps inside, wait in front, names), ns."""
    out, cur, prev_end = [], None, None
    for s, e, qu, n in ev:
        if qu != queue:
            continue
        if cur is None and first in n:
            cur = dict(sum=0, gaps=0, wait=(s - prev_end) if prev_end is not None else 0, names=[], end=None)
        if cur is not None:
            if cur["end"] is not None:
                cur["gaps"] += s - cur["end"]
            cur["sum"] += e - s
            cur["end"] = e
            cur["names"].append(n[-40:])
            if last in n:
                out.append(cur)
                cur = None
        prev_end = e
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    series = "--series" in sys.argv
    for d in args:
        ev = load(d)
        qm = queue_of(ev, "smooth_linear_kernel")
        # (the flow stream: the other queue with topology launches - the ground truth of the reset runs its IPCS kernels elsewhere)
        qf = queue_of([e for e in ev if e[2] != qm], "topology_kernel")
        sm = [e - s for s, e, qu, n in ev if "smooth_linear_kernel" in n]
        tf = [e - s for s, e, qu, n in ev if "topology_kernel" in n and qu == qf]
        tm = [e - s for s, e, qu, n in ev if "topology_kernel" in n and qu == qm]
        half = lambda a: a[len(a) // 2:]   # noqa: E731
        mean = lambda a: sum(a) / max(len(a), 1) / 1e3   # noqa: E731
        print(f"{d}: smooth_linear_kernel {mean(half(sm)):.1f} us ({len(sm)} launches), topology_kernel flow stream "
              f"{mean(half(tf)):.1f} us ({len(tf)}), main stream {mean(half(tm)):.1f} us ({len(tm)})")
        for label, queue, first, last in (("main", qm, "remesh", "mlp_head"), ("flow", qf, "topology_kernel", "at_correction")):
            ch = half(chains(ev, queue, first, last))
            if not ch:
                print(f"  {label} chain: not found")
                continue
            med = lambda k: statistics.median(c[k] for c in ch) / 1e3   # noqa: E731
            print(f"  {label} chain (queue {queue}, {len(ch[-1]['names'])} kernels, {len(ch)} chains): kernels {med('sum'):.1f} us, "
                  f"gaps inside {med('gaps'):.1f} us, wait in front {med('wait'):.1f} us, "
                  f"kernels + gaps {statistics.median(c['sum'] + c['gaps'] for c in ch) / 1e3:.1f} us")
        if series:
            print("  smooth_linear_kernel us:", " ".join(f"{x / 1e3:.1f}" for x in half(sm)))
            print("  topology_kernel (flow) us:", " ".join(f"{x / 1e3:.1f}" for x in half(tf)))


if __name__ == "__main__":
    main()
