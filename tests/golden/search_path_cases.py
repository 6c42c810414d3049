"""Writes tests/golden/path_cases_found.json: start positions on the directed maps (tests/path_cases.py) whose FIRST move is one no
generator produces often enough -- the three-point move (opposite-edge Type I, either orientation), contiguous-edge Type I (rare on MS-DFM fields), a move in which the lookahead
rejects the candidate that would have won, a walk that gets stuck after a real move.  Pure CPU: the oracle's extractor with its census
(oracle/ufm_path_oracle.c) on the oracle's final fields, over every point k/16 of every cell edge and every vertex of every map.

    python tests/golden/search_path_cases.py          # a minute or two; rewrites the json next to it
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import oracle_py as orc      # noqa: E402
import path_cases as pc      # noqa: E402

KEEP = 20                    # per (algo, target): enough for the floors (8 / 25 / 5) together with what the generators give


def candidates(cost):
    length, width = cost.shape
    for x in range(length + 1):
        for y in range(width + 1):
            yield (float(x), float(y))
            for k in range(1, 16):
                if x < length:
                    yield (x + k / 16.0, float(y))
                if y < width:
                    yield (float(x), y + k / 16.0)


def main():
    found, counts = [], {}
    for algo in ("FD", "SG", "DFM"):
        indirect = pc.INDIRECT[algo]
        targets = ["lookahead rejected the winner", "stuck after a move"] + (["opposite I h", "opposite I v", "contiguous I h", "contiguous I v"] if indirect else [])
        for name, cost, thr in pc.directed_maps():
            if all(counts.get((algo, t), 0) >= KEEP for t in targets):
                break
            rhs, tu = pc.oracle_field(algo, cost, thr)
            for start in candidates(cost):
                for la in (True, False):
                    orc.path_census_reset()
                    orc.extract_path_field(rhs, algo == "DFM", cost, tu, start, pc.GOAL, max_steps=2, lookahead=la, allow_indirect=indirect)
                    log = orc.path_move_log()
                    first = log[0]
                    hits = []
                    if first[2] == 2 and first[3] == 0:
                        hits.append("opposite I " + orc.PC_ORIENT[first[4]])
                    if first[2] == 1 and first[3] == 0:
                        hits.append("contiguous I " + orc.PC_ORIENT[first[4]])
                    if first[7] & 2:
                        hits.append("lookahead rejected the winner")
                    if len(log) > 1 and first[0] > 0 and log[1][0] == 0:
                        hits.append("stuck after a move")
                    for h in hits:
                        n = counts.get((algo, h), 0)
                        if n < KEEP:
                            counts[(algo, h)] = n + 1
                            found.append({"algo": algo, "map": name, "x": start[0], "y": start[1], "lookahead": int(la), "why": h})
    for k in sorted(counts):
        print(k, counts[k])
    with open(os.path.join(HERE, "path_cases_found.json"), "w") as f:
        json.dump({"made_by": "tests/golden/search_path_cases.py", "inputs": found}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
