#!/usr/bin/env python3
"""The table of profiles/chain_verdicts.txt: every stream of tests/test_gpu_chain_verdicts.py alone through the whole-GPU inflate, and
which chain delivered it (tests/chain_verdict.py reads the chains' control words; needs lib/libhdlz_dbg.so: csrc/build.sh dbg).
  python tools/chain_verdicts.py > profiles/chain_verdicts.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import hdl_deflate_amd                          # noqa: E402
import test_gpu_chain_verdicts as T             # noqa: E402

print("command: python tools/chain_verdicts.py > profiles/chain_verdicts.txt    (by: the chain that delivered the stream; the counters are "
      "those of the chain for any block types, - : not launched)")
for line in T.verdict_table(hdl_deflate_amd.Engine()):
    print(line, flush=True)
