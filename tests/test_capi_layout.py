"""The ctypes mirrors of the decode session's structs (pandepth_amd/capi.py) against include/pandepth_amd.h as the host compiler lays
it out: sizeof and every offsetof, field by field.  No GPU.  A mirror that is off by a field would make every call of
tests/test_gpu_decode_session.py hand the library something other than what the test wrote down."""
import ctypes
import os
import shutil
import subprocess

import pytest

from pandepth_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the fields as the header names them, in its order (written down here, not taken from the mirrors)
FIELDS = {
    "pd_bgzf_block": ["in_off", "out_off", "in_len", "out_len"],
    "pd_decode_cfg": ["flag_mask", "min_mapq", "contig_on", "span_off", "spans", "sorted", "bytes_hint", "batch_bytes", "batches_in_flight",
                      "flags", "n_batches"],
    "pd_decode_unit": ["start", "stop", "avail", "first_block", "n_blocks", "flags", "pad"],
    "pd_decode_batch": ["host_buf", "n_bytes", "blocks", "n_blocks", "pad", "inflated_bytes", "units", "n_units", "pad2", "order"],
    "pd_decode_result": ["n_reads", "n_first", "n_other", "first_start", "next_start", "ms_h2d", "ms_inflate", "ms_walk", "ms_emit",
                         "first_key", "last_key", "unsorted", "pad"],
}


@pytest.fixture(scope="module")
def header_layout(tmp_path_factory):
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc, "no host C compiler"
    d = tmp_path_factory.mktemp("layout")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pandepth_amd.h"', "int main(void) {"]
    for s, fields in FIELDS.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in fields:
            lines.append('    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f))
    lines += ["    return 0;", "}"]
    src = os.path.join(str(d), "layout.c")
    with open(src, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    exe = os.path.join(str(d), "layout")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode()
    size, offs = {}, {}
    for ln in out.splitlines():
        w = ln.split()
        if w[1] == "sizeof":
            size[w[0]] = int(w[2])
        else:
            offs[(w[0], w[1])] = (int(w[2]), int(w[3]))
    return size, offs


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_ctypes_mirror_has_the_headers_layout(header_layout, name):
    size, offs = header_layout
    mirror = getattr(capi, name)
    assert mirror in capi.DECODE_STRUCTS
    assert [f[0] for f in mirror._fields_] == FIELDS[name]
    assert ctypes.sizeof(mirror) == size[name], (name, ctypes.sizeof(mirror), size[name])
    for f in FIELDS[name]:
        d = getattr(mirror, f)
        assert (d.offset, d.size) == offs[(name, f)], (name, f, (d.offset, d.size), offs[(name, f)])


def test_every_field_of_the_header_is_listed():
    """the lists above against the header's text: a field added to one of the structs must be added here (and to the mirror)"""
    import re
    text = open(os.path.join(ROOT, "include", "pandepth_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name, fields in FIELDS.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        got = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                got.append(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1])
        assert got == fields, (name, got)
