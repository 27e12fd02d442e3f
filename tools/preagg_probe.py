"""What the sender-side collapse of identical descriptors (knob dist.preagg) does to one
rank's share of the sharded build's descriptor all-to-all. One rank of an N-rank C3 run holds 1/N
of the reads: mcaat_desc_preaggregate runs pass A, pass B and the collapse over that slice and
reports the live descriptors in, the (descriptor, weight) records out, and the records that left
raw; the shard_preagg stage time is the sender's cost. A record travels as 22 B (16-B descriptor,
2-B sub row, 4-B weight) against 18 B per slot pass A reserved without the collapse.
usage: python tools/preagg_probe.py --config c3 --fractions 8,4,2,1 [--repeat 3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mcaat_amd as M  # noqa: E402
from mcaat_amd.configs import CONFIGS  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--fractions", default="8,4,2,1")
    ap.add_argument("--repeat", type=int, default=3, help="runs per fraction (the first pays allocations)")
    ap.add_argument("--knob", action="append", default=[], help="name=value knob")
    a = ap.parse_args()
    cfg = CONFIGS[a.config]
    spec = cfg["spec"]
    with M.Context(0) as ctx:
        M.preload(ctx.device)
        for kv in a.knob:
            kn, kval = kv.split("=")
            ctx.set_knob(kn, int(kval))
        for n in [int(x) for x in a.fractions.split(",")]:
            r = M.Reads.synth_range(ctx, spec, 0, spec.n_reads // n)
            print(f"== 1/{n} of the reads ({spec.n_reads // n})", flush=True)
            for rep in range(a.repeat):
                ctx.reset_timing()
                d = M.desc_preaggregate(ctx, r, cfg["k"])
                st = ctx.stage_times()
                part = ctx.kernel_timing("preagg_partition")
                coll = ctx.kernel_timing("desc_preagg")
                hist = ctx.kernel_timing("l2_hist")
                print(f"   run {rep}: live in {d['live_in']} records out {d['records_out']} "
                      f"({d['records_out'] / max(1, d['live_in']):.4f}) raw {d['raw']} "
                      f"bytes out {22 * d['records_out'] / 1e9:.3f} GB | node_counter_a {st.get('node_counter_a', 0):.2f} ms "
                      f"shard_preagg {st.get('shard_preagg', 0):.2f} ms (l2_hist {hist[0] * hist[1]:.2f}, pass B "
                      f"{part[0] * part[1]:.2f} in {part[1]} groups, collapse {coll[0] * coll[1]:.2f})", flush=True)
            r.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
