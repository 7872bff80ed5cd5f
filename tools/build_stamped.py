#!/usr/bin/env python3
"""Diagnostic build (hipcc only, no GPU needed): the whole library with -DMMB_STAMPS into tools/_stamp/libmmbert_hip_stamps.so (git-ignored).
The stamp tools (stamp_attn.py) load THAT file; the product build (msa_amd/build.py) refuses every -DMMB_* define."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msa_amd.build import CSRC, FLAGS, HIPCC, SOURCES  # noqa: E402
OUT = os.path.join(ROOT, "tools", "_stamp")
os.makedirs(OUT, exist_ok=True)
procs, objs = [], []
for s in SOURCES:
    o = os.path.join(OUT, s.replace(".hip", "_stamps.o"))
    objs.append(o)
    procs.append(subprocess.Popen([HIPCC, *FLAGS, "-DMMB_STAMPS", "-c", os.path.join(CSRC, s), "-o", o]))
for p in procs:
    assert p.wait() == 0
lib = os.path.join(OUT, "libmmbert_hip_stamps.so")
subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs])
print(lib)
