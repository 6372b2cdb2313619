"""Every kernel of the LSTM sequence library (csrc/lg_lstm_seq.hip -> liblegged_lstm_seq.so) is compared with float64 by at least one GPU
test: the fifth coverage table, beside the step, actor, learner and tail kernels' (which read csrc/kernel_resources.txt).
csrc/kernel_resources_lstm_seq.txt (written by __graft_entry__.build()) lists what hipcc compiled for this library; the table below names,
for each symbol, the GPU test functions that dispatch it and compare its results with the float64 reference.  A new kernel or template
instantiation fails this test until a test for it is added to the table.  (CPU only: the module is parsed, not imported.)"""
import ast
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources_lstm_seq.txt")

GPU = "tests/test_gpu_lstm_sequence.py"
EDGES = "tests/test_gpu_lstm_sequence_edges.py"               # the table of tests/lstm_seq_check.py: 3 .. 7 waves, every k-step remainder, every staging regime
FORWARD = [f"{GPU}::test_forward_matches_float64_with_and_without_a_workspace", f"{GPU}::test_forward_with_weights_times_three_matches_float64",
           f"{GPU}::test_forward_through_a_strided_input_equals_the_contiguous_one", f"{GPU}::test_forward_matches_the_explicit_float64_restatement",
           f"{GPU}::test_saturated_gates_stay_finite_and_within_the_bars",
           f"{EDGES}::test_forward_gates_c_and_h_match_float64_element_by_element", f"{EDGES}::test_weights_times_three_match_float64_forward_and_backward",
           f"{EDGES}::test_the_forward_follows_the_parameters_on_one_handle"]
BACKWARD = [f"{GPU}::test_backward_matches_float64_autograd", f"{GPU}::test_backward_with_weights_times_three_matches_float64_autograd",
            f"{GPU}::test_saturated_gates_stay_finite_and_within_the_bars", f"{GPU}::test_outputs_are_written_everywhere_and_nothing_behind_them",
            f"{GPU}::test_module_with_sequence_attached_matches_float64_in_every_parameter_gradient",
            f"{EDGES}::test_backward_dG_matches_float64_element_by_element", f"{EDGES}::test_parameter_gradients_through_the_module_match_float64",
            f"{EDGES}::test_weights_times_three_match_float64_forward_and_backward"]
# a pack that misplaces a weight, or that does not run again after the parameters moved, shows in the forward's gates
PACK = [f"{GPU}::test_forward_matches_float64_with_and_without_a_workspace", f"{GPU}::test_backward_matches_float64_autograd",
        f"{EDGES}::test_forward_gates_c_and_h_match_float64_element_by_element", f"{EDGES}::test_the_forward_follows_the_parameters_through_the_module",
        f"{EDGES}::test_the_forward_follows_the_parameters_on_one_handle"]

COVERAGE = {
    "_ZN2lg14k_lstm_seq_fwdENS_14LstmSeqFwdArgsE": FORWARD,
    "_ZN2lg14k_lstm_seq_bwdENS_14LstmSeqBwdArgsE": BACKWARD,
    # every handle of the GPU tests packs on the device: a misplaced weight shows in the forward's comparison (odd and even K, 1 .. 8 waves:
    # test_every_wave_count_is_run below)
    "_ZN2lg15k_lstm_seq_packEPKfS1_S1_S1_P15HIP_vector_typeIfLj4EES4_iii": PACK,
}


def compiled(path=RESOURCES):
    names = set()
    with open(path) as f:
        for line in f:
            m = re.match(r"(\S+)\s", line)
            if m and not line.startswith("#"):
                names.add(m.group(1))
    return names


def uncovered(path=RESOURCES):
    return sorted(compiled(path) - set(COVERAGE))


def test_every_kernel_of_the_library_has_a_reference_test():
    names = compiled()
    assert len(names) == len(COVERAGE) == 3
    assert uncovered() == [], "kernels no GPU test compares with a reference: " + ", ".join(uncovered())
    assert set(COVERAGE) == names, "table entries for kernels that are no longer compiled: " + ", ".join(sorted(set(COVERAGE) - names))


def _test_functions(path):
    """The test functions of a module that is marked gpu as a whole, and the names it parametrises ``shape`` over."""
    with open(os.path.join(REPO, path)) as f:
        tree = ast.parse(f.read())
    gpu = any(isinstance(n, ast.Assign) and any(getattr(x, "id", None) == "pytestmark" for x in n.targets) and "gpu" in ast.unparse(n.value)
              for n in tree.body)
    assert gpu, f"{path} is not marked gpu"
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    over = {name: [ast.unparse(d.args[1]) for d in n.decorator_list if isinstance(d, ast.Call) and "parametrize" in ast.unparse(d.func)
                   and ast.unparse(d.args[0]) == "'shape'"] for name, n in funcs.items()}
    return funcs, over


def test_every_named_test_function_exists():
    funcs = {path: _test_functions(path)[0] for path in (GPU, EDGES)}
    for tests in COVERAGE.values():
        assert tests
        for t in tests:
            path, func = t.split("::")
            assert path in funcs and func in funcs[path], t


def test_every_wave_count_is_run():
    """The "1 .. 8 waves" of the table above: the first test named for each kernel in either module runs the module's whole shape list,
    and the two lists together hold every ``H / 32`` from 1 to 8, and odd and even K."""
    from tests import lstm_seq_check as lc
    lists = {GPU: ("SHAPES", lc.OLD_SHAPES), EDGES: ("lc.SHAPES", lc.SHAPES)}
    with open(os.path.join(REPO, GPU)) as f:
        assert "\nSHAPES = list(lc.OLD_SHAPES)\n" in f.read()
    for symbol, tests in COVERAGE.items():
        waves = set()
        for path, (name, shapes) in lists.items():
            over = _test_functions(path)[1]
            first = next(t.split("::")[1] for t in tests if t.startswith(path))
            assert over[first] == [name], (symbol, first, over[first])
            waves |= {(h // 32, (i + h) & 1) for _, _, i, h in shapes}
        assert {w for w, _ in waves} == set(range(1, 9)) and {odd for _, odd in waves} == {0, 1}, (symbol, sorted(waves))


def test_a_new_kernel_is_reported_uncovered(tmp_path):
    extra = ["_ZN2lg14k_lstm_seq_fwdILi16EEEvNS_14LstmSeqFwdArgsE", "_ZN2lg13k_lstm_seq_dwENS_13LstmSeqDwArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources_lstm_seq.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 128  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 2\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
