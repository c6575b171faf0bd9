"""The text of the generated kernels lives in files under csrc/kernels/ that the Makefile links in as strings (its TEXTS list): every
file of the list is there and can stand inside the raw string the rule wraps it in, the two host files that assemble the texts hold
no kernel text of their own, and no file of the list is dead -- each one's first line shows up in a text the library generates, once."""
import ctypes as C
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libxsmm-1_amd", "csrc")
TRANS_B = 2


def _makefile_texts():
    """-> ([(file, symbol)], the terminator of the raw string) as csrc/Makefile states them"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read().replace("\\\n", " ")
    entries = re.search(r"^TEXTS\s*:=(.*)$", mk, re.M).group(1).split()
    delimiters = set(re.findall(r'R"(\w+)\(', mk))
    assert len(delimiters) == 1 and all(")%s\"" % d in mk for d in delimiters), delimiters
    return [tuple(e.split(":")) for e in entries], ")%s\"" % delimiters.pop()


def _first_line(path):
    with open(path) as f:
        return next(line.rstrip("\n") for line in f if line.strip())


def test_every_listed_file_can_stand_in_the_raw_string():
    texts, terminator = _makefile_texts()
    assert len(texts) >= 11 and len(set(f for f, _ in texts)) == len(texts) == len(set(s for _, s in texts))
    for name, symbol in texts:
        path = os.path.join(CSRC, "kernels", name)
        assert os.path.isfile(path), name
        with open(path) as f:
            body = f.read()
        assert not re.search(r"^\s*#\s*include\b", body, re.M), name  # (hiprtc gets the text without include paths)
        assert terminator not in body and body.endswith("\n"), name
        assert re.fullmatch(r"[A-Z][A-Z0-9_]*", symbol), symbol


@pytest.mark.parametrize("host", ["xsmm_jit_smm.cpp", "xsmm_packed.cpp"])
def test_host_files_hold_no_kernel_text(host):
    with open(os.path.join(CSRC, host)) as f:
        src = f.read()
    assert not re.search(r'(?<![A-Za-z0-9_])(?:u8|u|U|L)?R"[^\s()\\]{0,16}\(', src)  # (a raw string literal: R"delimiter( ...)
    symbols = [s for _, s in _makefile_texts()[0] if re.search(r"\b%s\b" % s, src)]
    assert symbols, host  # (it uses texts of the list ...)
    for s in symbols:
        assert re.search(r"extern const char\* const %s;" % s, src), (host, s)  # (... and only declares them)


def _generated_texts(xs):
    """one text per form, compile == 0: {label: text}"""
    L = xs.lib()
    buf = C.create_string_buffer(1 << 21)
    out = {}

    def single(label, prec, shape, variant):
        blob, d = xs.descriptor(prec, *shape)
        n = L.libxsmm_amd_smm_kernel_source(d, variant, buf, len(buf), 0)
        out[label] = buf.value.decode()
        assert 0 < n == len(out[label]), label

    single("tiled_wave", xs.F64, (13, 13, 13), 0)
    single("tiled_wave_runs", xs.F64, (32, 32, 32), 1 | 2)
    single("tiled_wg_runs", xs.F64, (32, 32, 32), 1 | 4)
    single("mfma_wave", xs.F32, (36, 33, 12), 16384 | 1)
    single("mfma_wave2", xs.F64, (56, 56, 56), 32768)
    single("mfma_runs", xs.F64, (32, 32, 64), 65536 | 1 | 2)
    single("mfma_stream", xs.F64, (32, 32, 64), 65536 | 1)
    single("mfma_wg", xs.F32, (40, 40, 40), 64 | 128)
    single("big", xs.F64, (64, 64, 64), 16)
    keep = [xs.descriptor(xs.F64, m, m, m) for m in (13, 32)]
    arr = (C.c_void_p * 2)(*[C.cast(d, C.c_void_p) for _, d in keep])
    n = L.libxsmm_amd_smm_grouped_kernel_source(arr, 2, buf, len(buf), 0)
    out["grouped"] = buf.value.decode()
    assert 0 < n == len(out["grouped"]) and "namespace xg1 {" in out["grouped"]
    blob, d = xs.packed_descriptor(xs.KIND_PGEMM, 8, 8, 8, 8)
    n, out["packed_pgemm"] = xs.packed_kernel_source(xs.KIND_PGEMM, d, compile=0)
    assert 0 < n == len(out["packed_pgemm"])
    return out


def _scopes(text):
    """a text cut into the pieces within which a file may stand once: the per-shape namespaces of a grouped text and what is outside them"""
    cuts = [m.start() for m in re.finditer(r"^namespace xg\d+ \{$", text, re.M)]
    if not cuts:
        return [text]
    end = text.index("struct GroupEntry")
    bodies = [text[a:b] for a, b in zip(cuts, cuts[1:] + [end])]
    return [text[:cuts[0]] + text[end:]] + bodies


def test_no_listed_file_is_dead_or_doubled(xs):
    generated = _generated_texts(xs)
    texts, _ = _makefile_texts()
    for name, symbol in texts:
        line = _first_line(os.path.join(CSRC, "kernels", name)) + "\n"
        counts = {label: [scope.count(line) for scope in _scopes(text)] for label, text in generated.items()}
        assert any(sum(c) for c in counts.values()), "%s (%s) is in none of the generated texts" % (name, symbol)
        doubled = {label: c for label, c in counts.items() if max(c) > 1}
        assert not doubled, "%s (%s) stands twice in %r" % (name, symbol, doubled)
        assert counts["grouped"][0] == (1 if name in ("smm_jit_geom.h", "smm_jit_prelude.inc") else 0), name  # (file scope: once for all shapes)
