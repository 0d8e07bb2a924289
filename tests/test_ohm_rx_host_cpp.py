"""Builds and runs tests/cpp/test_receiver.cpp: the Songcast receiver in the host adapter (OhmReceiver).

Without a GPU: the queue's bookkeeping, and the element alone over scripted sessions -- the device call of every tick stood in for
by csrc/ohm_rx_core.h run on the CPU (the element's Collect / FillSource / Deliver around it).  What the element does, in order -- a
stream announced at NEW_STREAM with the wire's format, a delay in jiffies at DELAY, the audio cut into 5 ms messages at the right
track offsets, halt, stop, the resend datagram, what stays queued from tick to tick, what is ignored until Restart() -- is written to
a report and compared line by line with what the model (tests/ohm_rx_textbook.py) says must happen, tick by tick with the waiting
frames replayed in front.  With a GPU (tests/test_gpu_ohm_rx_to_driver.py) the same ticks go through OhmReceiver::Flush and the
bytes that reach ProcessorPcmBufTest are compared too."""
import os
import subprocess

import ohm_rx_cases as RC
import ohm_rx_textbook as RX
import ohm_textbook as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_receiver")
PER_SECOND = 56448000
PACKET_JIFFIES = 5 * 56448
RESTART = None


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_receiver.cpp")
    lib_dir = os.path.join(ROOT, "ohpipeline_amd", "lib")
    deps = [src, os.path.join(lib_dir, "libohhost.so"), os.path.join(lib_dir, "libohgpu.so"), os.path.join(ROOT, "ohpipeline_amd", "csrc", "ohm_rx_core.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE,
                           "-L", lib_dir, "-lohhost", "-lohgpu", f"-Wl,-rpath,{lib_dir}", "-lpthread"])
    return EXE


def songcast_ticks(rate):
    return (44100 if rate % 7350 == 0 else 48000) * 256


class LaneModel:
    """what OhmReceiver must do with a lane's arrivals, from the model: the report's lines and the bytes that reach the pipeline"""

    def __init__(self, index):
        self.i, self.state, self.queue, self.waiting = index, RX.new_state(), [], 0
        self.stopped, self.ignored, self.track, self.frames, self.bytes, self.out = False, 0, 0, 0, 0, bytearray()

    def line(self, lines, text):
        lines.append("%d %s" % (self.i, text))

    def push(self, gram):
        if gram is RESTART:
            self.stopped = False
        elif self.stopped:
            self.ignored += 1
        else:
            self.queue.append(gram)

    def flush(self, lines):
        if self.stopped or not self.queue:
            return
        recs, res, out = RX.receive(self.state, self.queue)
        fmt = None if self.state["stream_msg_due"] else (self.state["bit_depth"], self.state["channels"], self.state["sample_rate"])
        run = [0]

        def flush_run():
            depth, channels, rate = fmt
            per_sample = PER_SECOND // rate
            most = PACKET_JIFFIES // per_sample * channels * depth // 8
            done = 0
            while done < run[0]:
                piece = min(most, run[0] - done)
                jiffies = piece // (channels * depth // 8) * per_sample
                self.line(lines, "audio %d %d" % (self.track, jiffies))
                self.track += jiffies
                done += piece
            self.bytes += run[0]
            run[0] = 0

        for r in sorted((r for r in recs if r["disposition"] == RX.OUTPUT), key=lambda r: r["order"]):
            if r["events"] and fmt:
                flush_run()
            if r["events"] & RX.NEW_STREAM:
                per_sample = PER_SECOND // r["sample_rate"]
                self.line(lines, "stream %d %d %d %d [%s] %d %d %d" % (r["bit_rate"], r["bit_depth"], r["sample_rate"], r["channels"], r["codec"].decode(),
                                                                      r["samples_total"] * per_sample, r["sample_start"], 1 if r["flags"] & 2 else 0))
                self.track = r["sample_start"] * per_sample
                fmt = (r["bit_depth"], r["channels"], r["sample_rate"])
            if r["events"] & RX.DELAY:
                self.line(lines, "delay %d" % (r["media_latency"] * PER_SECOND // songcast_ticks(r["sample_rate"])))
            run[0] += r["audio_bytes"]
            self.frames += 1
            if r["events"] & RX.HALT:
                flush_run()
                self.line(lines, "halt")
        if fmt:
            flush_run()
        self.out += out
        self.state = res["state_out"]
        if res["stop_reason"]:
            self.queue, self.waiting, self.stopped = [], 0, True
            self.line(lines, "stopped %d" % res["stop_reason"])
            return
        keep = sorted((k for k, r in enumerate(recs) if r["disposition"] == RX.PENDING), key=lambda k: recs[k]["order"])
        self.queue, self.waiting = [self.queue[k] for k in keep], len(keep)
        if res["resend"]:
            self.line(lines, "resend " + RX.resend_datagram(res["resend"]).hex())


def expected(lanes):
    """lanes: [(arrivals with RESTART marks, datagrams per tick)] -> (the report's lines, the bytes per lane)"""
    models, lines, at, tick = [LaneModel(i) for i in range(len(lanes))], [], [0] * len(lanes), 0
    while True:
        for m, (arrivals, per_tick) in zip(models, lanes):
            for gram in arrivals[at[m.i]:at[m.i] + per_tick]:
                m.push(gram)
            at[m.i] += per_tick
        for m in models:
            m.flush(lines)
        for m in models:
            m.line(lines, "tick %d waiting %d queued %d stopped %d" % (tick, m.waiting, len(m.queue), 1 if m.stopped else 0))
        tick += 1
        if all(at[i] >= len(arrivals) for i, (arrivals, _) in enumerate(lanes)):
            break
    for m in models:
        m.line(lines, "end frames %d bytes %d ignored %d" % (m.frames, m.bytes, m.ignored))
    return lines, [bytes(m.out) for m in models]


def scripted_lanes():
    rng = RC.Lcg(91)

    def stereo16(frame, n=220, **more):
        return RC.audio_gram(frame & 0xffffffff, rng.bytes(4 * n), **more)

    # lane 0: 5 ms stereo frames, reordered within a few places with resent copies, three a tick: repairs span ticks
    order = RC.window_shuffle(list(range(40)), rng, reach=4)
    lane0 = []
    for j in order:
        lane0.append(stereo16(0xfffffff0 + j))
        if j % 7 == 3:
            lane0.append(stereo16(0xfffffff0 + j, n=1, flags=OT.FLAG_LOSSLESS | OT.FLAG_RESENT))
    # lane 1: a format change, a latency change, other message types, a halt that stops it, arrivals that are ignored, a restart
    lane1 = [RC.audio_gram(7, rng.bytes(6 * 240), depth=24, rate=48000, codec=b"FLAC", latency=9600, samples_total=10 ** 6, sample_start=480),
             RC.other_gram(4, b"a track"), RC.audio_gram(8, rng.bytes(6 * 240), depth=24, rate=48000, codec=b"FLAC", latency=9600, samples_total=10 ** 6, sample_start=720),
             RC.audio_gram(9, rng.bytes(6 * 100), depth=24, rate=48000, codec=b"FLAC", latency=4800, samples_total=10 ** 6, sample_start=960),
             RC.audio_gram(10, rng.bytes(2 * 441), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=0), b"junk",
             RC.audio_gram(12, rng.bytes(2 * 10), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=661),
             RC.audio_gram(11, rng.bytes(2 * 220), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=441, flags=OT.FLAG_HALT),
             RC.audio_gram(13, rng.bytes(2 * 10), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=671),
             RC.audio_gram(14, rng.bytes(2 * 10), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=681), RESTART,
             RC.audio_gram(15, rng.bytes(2 * 10), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=691),
             RC.audio_gram(3, rng.bytes(2 * 10), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=701),
             RC.audio_gram(16, rng.bytes(2 * 10), depth=16, channels=1, rate=44100, codec=b"", latency=4410, sample_start=711)]
    # lane 2: a gap that is never filled: the resend request every tick, then the reset when the window is left
    lane2 = [stereo16(f, n=50) for f in (1, 2, 4, 5, 30, 6, 7, 8)] + [stereo16(240, n=50), stereo16(241, n=50), stereo16(242, n=50)]
    return [(lane0, 3), (lane1, 2), (lane2, 2)]


def write_job(tmp_path, lanes):
    manifest = []
    for i, (arrivals, per_tick) in enumerate(lanes):
        stem = tmp_path / ("lane%d" % i)
        (tmp_path / ("lane%d.datagrams" % i)).write_bytes(b"".join(g for g in arrivals if g is not RESTART))
        (tmp_path / ("lane%d.sizes" % i)).write_text(" ".join("0" if g is RESTART else str(len(g)) for g in arrivals) + "\n")
        manifest.append("%s %d" % (stem, per_tick))
    (tmp_path / "job.txt").write_text("\n".join(manifest) + "\n")
    return str(tmp_path / "job.txt")


def run(mode, tmp_path, lanes):
    exe = build_test_binary()
    args = [exe, mode, write_job(tmp_path, lanes), str(tmp_path / "report.txt")] + ([str(tmp_path / "bytes.bin")] if mode == "gpu" else [])
    out = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    return (tmp_path / "report.txt").read_text().splitlines()


def test_the_script_covers_what_it_is_meant_to():
    lines, outs = expected(scripted_lanes())
    kinds = {(int(l.split()[0]), l.split()[1]) for l in lines}
    assert {(0, "stream"), (0, "audio"), (0, "resend"), (1, "delay"), (1, "halt"), (1, "stopped"), (2, "resend")} <= kinds
    assert sum(1 for l in lines if l.startswith("1 stream")) == 3 and "1 stopped 2" in lines and "1 stopped 1" in lines
    assert any(l.startswith("0 tick") and " waiting 0" not in l for l in lines)          # a repair that spans a tick
    assert len(outs[0]) == 40 * 880 and lines[-2].endswith("ignored 2")
    assert [l for l in lines if l.startswith("0 audio")][0] == "0 audio %d %d" % (((0xfffffff0 + 0x200) & 0xffffffff) * 220 * 1280, 220 * 1280)


def test_the_element_alone_over_the_core_on_the_cpu(tmp_path):
    lanes = scripted_lanes()
    want, _ = expected(lanes)
    got = run("cpu", tmp_path, lanes)
    assert got == want, next(("line %d: got %r, want %r" % (k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w), "lengths %d, %d" % (len(got), len(want)))
