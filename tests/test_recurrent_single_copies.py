"""The recurrent libraries are written once (no GPU): each shared device body and host helper has ONE home under csrc/, and the nine
libraries are one table in ``capi`` (``LIBRARIES``) and one in ``__graft_entry__`` (``LIBS``) from which every public name is derived."""
import os
import re

import pytest

import __graft_entry__ as entry
from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CSRC = os.path.join(REPO, "legged_games_gym_amd", "csrc")

# record -> (the prefix of load_<p>library / <p>library_path / bind_<q>, the names of its tables in capi, the prefix of its names in entry)
NAMES = {
    "main": ("", "all", None, "ALL_SYMBOLS", "HIP"),
    "lstm_seq": ("lstm_seq_", "lstm_seq", "LSTM_SEQ_ABI", "LSTM_SEQ_SYMBOLS", "SEQ"),
    "game_recurrent": ("game_recurrent_", "game_recurrent", "GAME_RECURRENT_ABI", "GAME_RECURRENT_SYMBOLS", "GAME_REC"),
    "dec_game_recurrent": ("dec_game_recurrent_", "dec_game_recurrent", "DEC_GAME_RECURRENT_ABI", "DEC_GAME_RECURRENT_SYMBOLS", "DEC_GAME_REC"),
    "dec_pool_recurrent": ("dec_pool_recurrent_", "dec_pool_recurrent", "DEC_POOL_RECURRENT_ABI", "DEC_POOL_RECURRENT_SYMBOLS", "DEC_POOL_REC"),
    "dec_game_privileged": ("dec_game_privileged_", "dec_game_privileged", "DEC_GAME_PRIVILEGED_ABI", "DEC_GAME_PRIVILEGED_SYMBOLS", "DEC_GAME_PRIV"),
    "lstm_wide": ("lstm_wide_", "lstm_wide", "LSTM_WIDE_ABI", "LSTM_WIDE_SYMBOLS", "LSTM_WIDE"),
    "gru": ("gru_", "gru", "GRU_ABI", "GRU_SYMBOLS", "GRU"),
    "dec_game_gru": ("dec_game_gru_", "dec_game_gru", "DEC_GAME_GRU_ABI", "DEC_GAME_GRU_SYMBOLS", "DEC_GAME_GRU"),
}


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}


@pytest.mark.parametrize("text, home", [
    ("xs[k * LG_LSTM_LD + row]", "lg_lstm_cell_body.h"),            # the staging store of [x | h_in]: stage_xh
    ("#define LG_LSTM_KSTEP", "lg_lstm_cell_body.h"),               # the LSTM k-step: lstm_units
    ("vsnprintf(g_error", "lg_lib_error.h"),                        # refuse() of the single-unit libraries
    ("raise_lds_limit(const void", "lg_lib_error.h"),
    ("hipMemcpy(raw, w_ih", "lg_memory_host.h"),                    # the upload of a create: memory_create
])
def test_one_home_under_csrc(text, home):
    holders = [f for f, body in _sources().items() if text in body]
    assert holders == [home], (text, holders)
    assert _sources()[home].count(text) == 1, text


def test_the_sequence_library_keeps_its_own_error_sink_and_the_main_library_its_own():
    src = _sources()
    assert "seq_fail" in src["lg_lstm_seq.hip"] and '"lg_lib_error.h"' not in src["lg_lstm_seq.hip"]
    assert '"lg_lib_error.h"' not in src["lg_recurrent.hip"] and "fail(code" in src["lg_recurrent.hip"]      # the main library's sink: lg::fail
    seven = [f for f, body in src.items() if f.endswith(".hip") and '#include "lg_lib_error.h"' in body]
    assert seven == ["lg_dec_game_lstm_act.hip", "lg_dec_game_privileged.hip", "lg_dec_gru.hip", "lg_dec_pool_lstm_act.hip", "lg_game_lstm_act.hip",
                     "lg_gru.hip", "lg_lstm_wide.hip"]
    for f in seven:                                                  # the shared header is the only definition of HIP_TRY these units see last
        assert "#define HIP_TRY" not in src[f], f


def test_the_tables_hold_the_same_nine_libraries():
    assert list(capi.LIBRARIES) == list(NAMES) == [spec.key for spec in entry.LIBS]
    for spec in entry.LIBS:
        rec = capi.LIBRARIES[spec.key]
        assert os.path.basename(spec.target) == rec.file and getattr(capi, spec.symbols) == list(rec.abi), spec.key
        assert set(spec.checks) <= {"step_scratch", "no_spill", "two_waves"} and spec.checks, spec.key
    assert len({rec.file for rec in capi.LIBRARIES.values()}) == len({rec.env for rec in capi.LIBRARIES.values()}) == 9


@pytest.mark.parametrize("key", list(NAMES))
def test_public_names_come_from_the_record(key, monkeypatch, tmp_path):
    stem, bind_stem, abi, symbols, _ = NAMES[key]
    rec = capi.LIBRARIES[key]
    path_alias, load_alias, bind_alias = getattr(capi, stem + "library_path"), getattr(capi, f"load_{stem}library"), getattr(capi, "bind_" + bind_stem)
    # the tables of the record are the public ones
    assert getattr(capi, symbols) == list(rec.abi)
    if abi is not None:
        assert getattr(capi, abi) is rec.abi
    if rec.sizeof is not None:
        sizeof, structs = rec.sizeof
        assert sizeof in rec.abi and sizeof.endswith("_sizeof")
        assert dict(structs) == dict(enumerate(s) if isinstance(s := getattr(capi, symbols[:-len("SYMBOLS")] + "STRUCTS"), tuple) else s)
    # path: the in-tree file, or what the environment variable names
    monkeypatch.delenv(rec.env, raising=False)
    assert path_alias() == capi.path(key) == os.path.join(CSRC, rec.file)
    absent = str(tmp_path / ("absent_" + rec.file))
    monkeypatch.setenv(rec.env, absent)
    assert path_alias() == capi.path(key) == absent
    # load: the record's cache, and a loud refusal of a file that is not there
    marker = object()
    monkeypatch.setattr(rec, "handle", marker)
    assert load_alias() is marker and capi.load(key) is marker and getattr(capi, rec.cache) is marker
    monkeypatch.setattr(capi, rec.cache, None)                       # the module attribute is the record's cache: resetting either resets both
    assert rec.handle is None
    monkeypatch.setattr(rec, "handle", marker)
    monkeypatch.setattr(rec, "handle", None)
    assert getattr(capi, rec.cache) is None
    with pytest.raises(RuntimeError, match=r"is not built; run .*build\(\)") as refused:
        load_alias()
    assert absent in str(refused.value) and "no CPU fallback" in str(refused.value) and rec.handle is None
    # bind: the alias binds this record's entry points
    class Fn:
        argtypes = restype = None

    class Lib:
        pass
    lib = Lib()
    for symbol in rec.abi:
        setattr(lib, symbol, Fn())
    if key != "main" and rec.sizeof is None:                         # (a sizeof needs the real library: the per-library ABI tests bind it)
        assert bind_alias(lib) is lib
        for symbol, (argtypes, restype) in rec.abi.items():
            assert getattr(lib, symbol).argtypes == argtypes and getattr(lib, symbol).restype == restype, symbol


def _includes(path, seen=None, deep=True):
    """Base names of the ``#include "..."`` of ``path``; with ``deep`` also of every header reached from there."""
    seen = set() if seen is None else seen
    for inc in re.findall(r'#include\s+"([^"]+)"', open(path).read()):
        at = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if os.path.basename(at) not in seen:
            seen.add(os.path.basename(at))
            if deep:
                _includes(at, seen)
    return seen


@pytest.mark.parametrize("key", list(NAMES))
def test_header_lists_are_the_includes_of_the_source(key):
    """A library's header list is what its staleness check reads: it holds every header a source names, and no header that no source
    reaches.  (The main library's is every header no side library owns.)"""
    spec = next(s for s in entry.LIBS if s.key == key)
    prefix = NAMES[key][4]
    listed = {os.path.basename(h) for h in spec.headers}
    assert len(listed) == len(spec.headers), "a header listed twice"
    for h in spec.headers:
        assert os.path.isfile(h if os.path.isabs(h) else os.path.join(CSRC, h)), h
    direct, reached = set(), set()
    for source in spec.sources:
        direct |= _includes(os.path.join(CSRC, source), deep=False)
        reached |= _includes(os.path.join(CSRC, source))
    assert direct <= listed, direct - listed
    if key == "main":
        owned = {os.path.basename(h) for s in entry.LIBS for h in s.own_headers}
        assert listed == {f for d in (CSRC, entry.INCLUDE) for f in os.listdir(d) if f.endswith(".h")} - owned
        assert (entry.HIP_LIB, entry.HIP_SOURCES, entry.HIP_HEADERS, entry.RESOURCES) == (spec.target, spec.sources, spec.headers, spec.resources)
        return
    assert listed <= reached, listed - reached
    # the module attributes are the record's
    assert getattr(entry, prefix + "_LIB") == spec.target and getattr(entry, prefix + "_SOURCE") == spec.sources[0] and len(spec.sources) == 1
    assert getattr(entry, prefix + "_HEADERS") == spec.headers and getattr(entry, prefix + "_RESOURCES") == spec.resources
    if key != "lstm_seq":
        assert getattr(entry, prefix + "_OWN_HEADERS") == spec.own_headers
    for shared in ("lg_lib_error.h", "lg_memory_host.h"):           # the shared host headers are listed exactly where they are included
        assert (shared in listed) == (shared in direct), (key, shared)


def test_memory_kinds_name_their_library_and_entry_points():
    from legged_games_gym_amd.rl import recurrent_actor as ra
    assert set(ra.MEMORY_KINDS) == {"lstm", "lstm_wide", "gru"}
    for kind, (record, prefix, last_error, _) in ra.MEMORY_KINDS.items():
        abi = capi.LIBRARIES[record].abi
        assert last_error in abi, kind
        for entry_point in ("_create", "_load_device", "_destroy", "_step"):
            assert prefix + entry_point in abi, (kind, entry_point)
    assert issubclass(ra.DeviceLstm, ra.DeviceMemory) and issubclass(ra.DeviceGru, ra.DeviceMemory)
