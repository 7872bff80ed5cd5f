"""The build's source list against the source directory (no compile, no GPU): msa_amd/build.py ``SOURCES`` is the only list of the
library's sources (the tools read it), so it must name every ``*.hip`` of msa_amd/csrc and nothing else -- a file outside the list would
otherwise only surface as a missing symbol -- and every one of them includes include/mmbert_hip.h, so that the compiler holds each
entry point's definition to its prototype."""
import os

from msa_amd import build


def _hip_files():
    return sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))


def test_sources_are_the_hip_files_of_csrc():
    assert build.SOURCES == _hip_files()


def test_every_source_includes_the_contract():
    for name in _hip_files():
        text = open(os.path.join(build.CSRC, name)).read()
        assert '#include "../../include/mmbert_hip.h"' in text, name
