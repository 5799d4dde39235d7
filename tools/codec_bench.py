#!/usr/bin/env python3
"""The GF(2^8) codec forms of one geometry, timed against each other in one run.

For (n, f) one context is created per codec form available there -- the matrix
product, the specialised additive FFT (the RBC_FFT_GEOMS geometries), the
run-time-geometry additive FFT (33 <= n <= 128), its wide form
(129 <= n <= 256) or its small form (2 <= n <= 32), the last once per lane
width of --lane as "fft_small@<lane>" -- and three device calls are
timed with events on --instances values of --value-bytes each:

  encode   rbc_dev_encode alone
  commit   rbc_dev_shard_commit (encode, leaf hashes, Merkle build)
  receive  rbc_dev_verify + rbc_dev_interpolate(leaves_verified = 1) with n - f
           rows present per instance and the ECHO of 10 % of the instances
           corrupted; every row the receiver must regenerate is poisoned before
           each iteration (outside the timed span), so every iteration decodes

Every form first runs every call --warmup times; then the forms alternate,
iteration by iteration, for --iters (>= 20) timed iterations each.  Before
anything is reported the forms' outputs on the timed inputs are compared on the
device: encoded shards, roots, branches, statuses, values and digests must be
identical.  The result is one JSON line: per call and form the median, min, max
and every iteration in ms, and per call whether the generic (or wide, or small)
form's range lies wholly below or above the matrix codec's (and the specialised
one's), and the small form's wider lane against its lane 1.

  python tools/codec_bench.py --n 100 --f 33 --out profiles/fft_any/n100_f33.json
  python tools/codec_bench.py --all --out-dir profiles/fft_any
  python tools/codec_bench.py --n 200 --f 66 --instances 256 --out profiles/fft_wide/n200_f66.json
  python tools/codec_bench.py --n 19 --f 6 --out profiles/fft_small/n19_f6_1m.json
  python tools/codec_bench.py --n 19 --f 6 --value-bytes 16384 --lane 1 --out profiles/fft_small/n19_f6_16k.json

--all runs the geometries of DESIGN.md 5.1's table, each in a child process of
its own under its own time limit, and stops at the first that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMS = [(64, 20), (100, 33), (128, 30), (200, 66), (128, 42), (256, 85)]
CALLS = ("encode", "commit", "receive")


def rup(x, a):
    return (x + a - 1) // a * a


class Form:
    """One codec form's context and its own device buffers."""

    def __init__(self, ca, np, a, codec, values, present, corrupt):
        self.ca, self.np, self.codec = ca, np, codec  # codec: a set_codec name, or "fft_small@<lane>"
        self.ctx = ctx = ca.Context(a.n, a.f)
        name, _, lane = codec.partition("@")
        ctx.set_codec(name)
        if lane:
            ctx.set_fft_lane(int(lane))
        self.form = ctx.fft_form
        n, k, I = a.n, ctx.k, a.instances
        self.n, self.k, self.I, self.B = n, k, I, a.value_bytes
        self.S = S = (self.B + k - 1) // k
        self.sp, self.vp, self.op = rup(S, 64), values.shape[1], rup(k * S, 16)
        mb = ca.DeviceBuffer
        d = max(ctx.depth, 1)
        self.b = dict(values=mb(values.nbytes), shards=mb(I * n * self.sp), leaves=mb(I * n * 32), roots=mb(I * 32),
                      branches=mb(I * n * d * 32), present=mb(I * n), corrupt=mb(I * 4), valid=mb(I * n),
                      leaves_r=mb(I * n * 32), out=mb(I * self.op), digests=mb(I * 32), status=mb(I * 4))
        self.b["values"].upload(values)
        self.b["present"].upload(present)
        self.b["corrupt"].upload(corrupt)
        self.st = ca.Stream()
        self.ms = {c: [] for c in CALLS}

    def encode(self):
        b = self.b
        self.ctx.dev_encode(self.st.ptr, self.I, b["values"], self.vp, None, self.B, b["shards"], self.sp)

    def commit(self):
        b = self.b
        self.ctx.dev_shard_commit(self.st.ptr, self.I, b["values"], self.vp, None, self.B, b["shards"], self.sp, None,
                                  b["leaves"], b["roots"], b["branches"])

    def damage(self):
        """Untimed: garbage over every absent row and every corrupted ECHO."""
        b = self.b
        self.ca.rbc.poison_rows(0, self.st.ptr, b["shards"], self.n * self.sp, self.sp, self.n, b["present"],
                                b["corrupt"], self.I, 99)

    def receive(self):
        b, c = self.b, self.ctx
        c.dev_verify(self.st.ptr, self.I, b["shards"], self.sp, None, self.S, b["branches"], b["roots"], b["present"],
                     b["valid"], b["leaves_r"])
        c.dev_interpolate(self.st.ptr, self.I, b["shards"], self.sp, None, self.S, b["valid"], b["leaves_r"], 1,
                          b["roots"], b["out"], self.op, b["digests"], b["status"])

    def run(self, call, timed):
        if call == "receive":
            self.damage()
        e0, e1 = self.ca.Event(), self.ca.Event()
        e0.record(self.st)
        getattr(self, call)()
        e1.record(self.st)
        self.st.sync()
        if timed:
            self.ms[call].append(e0.elapsed_ms(e1))


def mismatches(ca, np, x, y, name, rows, length, pitch):
    counter = ca.DeviceBuffer(16)
    counter.zero()
    ca.rbc.count_mismatch(0, None, x.b[name], pitch, y.b[name], pitch, rows, length, counter)
    ca.rbc.lib.rbc_device_sync(0)
    return int(np.frombuffer(counter.download(4).tobytes(), np.uint32)[0])


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iters_ms": ms}


def verdict(a, b):
    """a against b by their min-max ranges: "faster", "slower", or "within the spread"."""
    if a["max_ms"] < b["min_ms"]:
        return "faster"
    if a["min_ms"] > b["max_ms"]:
        return "slower"
    return "within the spread"


def one(a):
    import numpy as np

    import cleisthenes_amd as ca

    assert ca.device_count() > 0, "no GPU visible"
    probe = ca.Context(a.n, a.f)
    k = probe.k
    codecs = ["matrix"]
    probe.set_codec("auto")
    if probe.fft_form == "specialised":
        codecs.append("fft")
    for codec in ("fft_generic", "fft_wide"):  # the run-time-geometry form built for this n, if any
        try:
            probe.set_codec(codec)
            codecs.append(codec)
        except ca.RBCError:
            pass
    small = []
    try:
        probe.set_codec("fft_small")
        for lane in a.lane if a.lane else (1, 2, 4):  # default: every lane width built for this n
            try:
                probe.set_fft_lane(lane)
                small.append(f"fft_small@{lane}")
            except ca.RBCError:
                if a.lane:
                    raise SystemExit(f"codec_bench: lane {lane} is not built for n = {a.n}")
    except ca.RBCError:
        pass
    codecs += small
    S = (a.value_bytes + k - 1) // k
    rng = np.random.default_rng(a.seed)
    values = rng.integers(0, 256, (a.instances, rup(k * S + 32, 64)), dtype=np.uint8)
    present = np.zeros((a.instances, a.n), np.uint8)
    corrupt = np.full(a.instances, -1, np.int32)
    for i in range(a.instances):
        pres = rng.permutation(a.n)[: a.n - a.f]
        present[i, pres] = 1
        if rng.random() < 0.10:
            corrupt[i] = int(rng.choice(pres))
    forms = [Form(ca, np, a, c, values, present, corrupt) for c in codecs]
    for call in CALLS:
        for _ in range(a.warmup):
            for fm in forms:
                fm.run(call, False)
        for _ in range(a.iters):
            for fm in forms:  # the forms alternate inside one process
                fm.run(call, True)
    # the outputs of the last timed iteration of every call, form against form
    ref, I, n = forms[0], a.instances, a.n
    for fm in forms[1:]:
        d = max(ref.ctx.depth, 1)
        bad = {"shards": mismatches(ca, np, ref, fm, "shards", I * n, S, ref.sp),
               "roots": mismatches(ca, np, ref, fm, "roots", I, 32, 32),
               "branches": mismatches(ca, np, ref, fm, "branches", I * n, d * 32, d * 32),
               "values": mismatches(ca, np, ref, fm, "out", I, k * S, ref.op),
               "digests": mismatches(ca, np, ref, fm, "digests", I, 32, 32),
               "status": mismatches(ca, np, ref, fm, "status", 1, I * 4, I * 4)}
        if any(bad.values()):
            raise SystemExit(f"codec_bench: {fm.codec} differs from matrix at ({a.n}, {a.f}): {bad}")
    status = np.frombuffer(ref.b["status"].download().tobytes(), np.int32)
    if (status != 0).any():
        raise SystemExit(f"codec_bench: {int((status != 0).sum())} instances did not decode")
    res = {"n": a.n, "f": a.f, "k": k, "instances": a.instances, "value_bytes": a.value_bytes, "shard_len": S,
           "warmup": a.warmup, "iters": a.iters, "corrupted_instances": int((corrupt >= 0).sum()),
           "forms": {fm.codec: fm.form for fm in forms}, "outputs_identical": True,
           "library": os.path.basename(ca.rbc.library_path()),
           "calls": {c: {fm.codec: stats(fm.ms[c]) for fm in forms} for c in CALLS}, "verdicts": {}}
    for c in CALLS:
        t = res["calls"][c]
        v = {}
        for codec, name in (("fft_generic", "generic"), ("fft_wide", "wide")):
            if codec not in t:
                continue
            v[f"{name}_vs_matrix"] = verdict(t[codec], t["matrix"])
            v[f"matrix_over_{name}_median"] = t["matrix"]["median_ms"] / t[codec]["median_ms"]
            if "fft" in t:
                v[f"{name}_vs_specialised"] = verdict(t[codec], t["fft"])
                v[f"{name}_over_specialised_median"] = t[codec]["median_ms"] / t["fft"]["median_ms"]
        for codec in small:
            v[f"{codec}_vs_matrix"] = verdict(t[codec], t["matrix"])
            v[f"matrix_over_{codec}_median"] = t["matrix"]["median_ms"] / t[codec]["median_ms"]
            if "fft" in t:
                v[f"{codec}_vs_specialised"] = verdict(t[codec], t["fft"])
                v[f"{codec}_over_specialised_median"] = t[codec]["median_ms"] / t["fft"]["median_ms"]
            if codec != "fft_small@1" and "fft_small@1" in t:
                v[f"{codec}_vs_fft_small@1"] = verdict(t[codec], t["fft_small@1"])
                v[f"fft_small@1_over_{codec}_median"] = t["fft_small@1"]["median_ms"] / t[codec]["median_ms"]
        res["verdicts"][c] = v
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=100)
    p.add_argument("--f", type=int, default=33)
    p.add_argument("--instances", type=int, default=1024)
    p.add_argument("--value-bytes", type=int, default=1 << 20)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--seed", type=int, default=20261020)
    p.add_argument("--lane", type=int, nargs="*", default=None,
                   help="the small form's lane widths to run (default: 1 and the wider one built for n)")
    p.add_argument("--out", default=None)
    p.add_argument("--all", action="store_true", help="every geometry of DESIGN.md 5.1's table, one child each")
    p.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "fft_any"))
    p.add_argument("--timeout", type=int, default=240, help="--all: seconds per geometry")
    a = p.parse_args()
    if a.iters < 20 or a.warmup < 1:
        p.error("at least 20 timed iterations and one warm-up")
    if not a.all:
        return one(a)
    for n, f in GEOMS:
        inst = min(a.instances, 256) if n >= 200 else a.instances  # 256 instances of 1 MiB from N = 200
        out = os.path.join(a.out_dir, f"n{n}_f{f}.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--f", str(f), "--instances", str(inst),
               "--value-bytes", str(a.value_bytes), "--warmup", str(a.warmup), "--iters", str(a.iters),
               "--seed", str(a.seed), "--out", out]
        r = subprocess.run(cmd, timeout=a.timeout)  # a child that hangs is killed; nothing is started after it
        if r.returncode != 0:
            raise SystemExit(f"codec_bench: ({n}, {f}) failed with status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
