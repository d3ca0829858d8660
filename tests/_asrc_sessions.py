"""Helper of test_gpu_asrc.py: plays fixed any-ratio sessions (the general kernel: BASELINE.json configs[4]'s stereo ASRC stream and its
neighbours — mono, short and long filters, wider streams below the pipelined loop's threshold) on two twin contexts in one process and
prints one sha256 per session and twin: single calls (the lean tap loop for one and two channels) against the same calls made as
batches of one (the plain loop) — _general_sessions.play.  Every block is played as calls of at most 45 T frames (what a batched
call takes: _general_sessions.pieces), so configs[4]'s 65,536-frame blocks arrive as calls of 17,100 frames; those make tiles of
one pass, and the sessions at 988 taps and at a ratio near 3 are there so that every lean form also runs tiles of several."""
import json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from _general_sessions import pieces, play
from _oracle import noise, BH, INTERP, LOWPASS, PRECISE

R = 48000 / 44100
SESSIONS = [
    # (channels, taps, filters, ratios per block, flags, blocks, kernel preference)
    (2, 380, 380, [R * (1 + 100e-6 * math.sin(2 * math.pi * i / 5 + 0.3)) for i in range(5)], BH, (65536, 30000, 65536, 1000, 40000), 0),    # BASELINE configs[4]'s stream, its blocks cut as above
    (2, 380, 380, [R * 1.00003] * 3, BH | INTERP, (50000, 4096, 33000), 0),                 # interpolating: rows fi and fi + 1, the last of a cell from the next
    (1, 988, 988, [R * 0.99991] * 2, BH | INTERP, (70000, 25000), 0),                       # mono, preset -4
    (1, 988, 988, [1.3700013] * 2, BH, (60000, 20000), 0),
    (2, 156, 156, [0.731] * 2, BH | INTERP, (90000, 30000), 0),                             # down-sampling: long input span per output range
    (2, 380, 64, [2.0 * 1.000013] * 2, BH, (40000, 20000), 0),                              # nearest filter without a low-pass, near a 2x ratio: pass-through outputs among the others
    (2, 380, 380, [R * 1.00002] * 2, BH | INTERP | PRECISE, (40000, 20000), 0),             # double accumulators
    (2, 512, 512, [R * 1.0000001] * 2, BH | INTERP, (60000, 30000), 0),                       # all but a rational ratio
    (2, 380, 380, [R * 1.00004] * 2, BH | INTERP | LOWPASS, (40000, 18000), 0),
    (8, 380, 380, [R * 1.00002] * 2, BH | INTERP, (20000, 6000), 0),                        # wider streams below the pipelined loop's 512 taps
    (4, 256, 256, [0.9131] * 2, BH, (20000, 6000), 0),                                      # 16 lanes per output
    (1, 16, 16, [1.0713] * 2, BH | INTERP, (30000, 5000), 0),                               # a filter shorter than a lane group
    (2, 48, 48, [R * 1.0001] * 2, BH | INTERP, (50000, 7000), 0),
    (3, 988, 988, [1.0000317] * 2, BH | INTERP, (9000, 3000), 0),
    (16, 156, 156, [R * 0.9999] * 2, BH | INTERP, (12000, 3000), 0),
    # stereo sessions whose calls make tiles of several passes in every lean form (LEAN 2: a wave's later outputs load their first round in the loop)
    (2, 988, 988, [R * 1.00001] * 2, BH | INTERP, (60000, 30000), 0),                       # 32 lanes per output: 40-output tiles of 8-output passes
    (2, 380, 380, [3.0 * 1.00002] * 2, BH | INTERP, (30000, 12000), 0),                     # up-sampling by ~3: 48-output tiles of 16-output passes
    (2, 380, 380, [3.0 * 0.99997] * 2, BH | INTERP | PRECISE, (30000, 12000), 0),           # the same with double accumulators
]


def main():
    out = {"single": [], "batched": []}
    for ch, T, F, ratios, flags, blocks, pref in SESSIONS:
        x, _ = noise(sum(blocks) * ch, state=(ch * 1000 + T + F) | 1)
        calls = [(p, ratios[i % len(ratios)]) for i, n in enumerate(blocks) for p in pieces(n, T)]
        for side, rec in zip(("single", "batched"), play(ch, T, F, flags, pref, x.reshape(-1, ch), calls)):
            out[side].append({"session": [ch, T, F, ratios[0]], **rec})
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
