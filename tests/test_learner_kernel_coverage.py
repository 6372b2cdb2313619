"""Every compiled instantiation of the learner kernels -- the wide MLP GEMMs and their helpers (csrc/lg_gemm.h), the chain forward
(csrc/lg_policy.h), the LDS-resident trainer (csrc/lg_train.h) and the PPO loss -- is compared with a reference by at least one GPU
test.  csrc/kernel_resources.txt (written by __graft_entry__.build()) lists what hipcc compiled; the table below names, for each
instantiation, the GPU test functions that dispatch it and compare its results with autograd / a float64 restatement.  A new template
instantiation fails this test until a test for it is added to the table.  (CPU only: the modules are parsed, not imported.)"""
import ast
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")

KERNELS = ("k_gemm_wide", "k_gemm_wide_bf16x3", "k_wide_prep", "k_wide_reduce", "k_wide_out_bwd",
           "k_mlp_chain_fwd64", "k_chain_pack", "k_mlp_train", "k_mlp_reduce", "k_ppo_loss")

RL, WIDE, FLAT64 = "tests/test_gpu_rl.py", "tests/test_gpu_wide_learner.py", "tests/test_gpu_flat_learner.py"
ROUGH = f"{RL}::test_wide_mlp_kernels_match_autograd"                      # 235 / 169 inputs, 12 / 1 outputs, mb 24 576 / 1000 / 37, both precisions
GENERIC = f"{WIDE}::test_wide_kernels_match_float64_autograd_on_the_generic_path"      # game shapes and the shapes around them, both precisions
STEP = f"{WIDE}::test_composed_minibatch_step_matches_float64_autograd_at_the_game_shape"
FLAT = f"{RL}::test_mlp_kernels_match_autograd"                            # 48-128-64-32 networks against autograd
RAGGED = f"{RL}::test_mlp_kernels_ragged_widths_and_a_single_net"
# compares two paths of the library (in-kernel loss against forward -> lg_ppo_loss -> backward): the float64 tests below are the reference tests
MINIBATCH = f"{RL}::test_fused_ppo_minibatch_equals_forward_loss_backward"
# 48-128-64-32 networks against float64 at the kernels' edges: widths, row-tile schedule and partial counts, gathers with repeated rows
FLAT_FB = [f"{FLAT64}::test_forward_and_backward_match_float64_over_widths", f"{FLAT64}::test_forward_and_backward_match_float64_over_the_schedule",
           f"{FLAT64}::test_gather_with_duplicates_and_table_ends"]
# ... and the build with the PPO loss inside: 1 .. 16 actions, the schedule, ratios far outside the clip range
FLAT_FUSED = [f"{FLAT64}::test_fused_minibatch_matches_float64_over_action_counts", f"{FLAT64}::test_fused_minibatch_matches_float64_over_the_schedule",
              f"{FLAT64}::test_fused_minibatch_far_outside_the_clip_range"]
# the chain forward against float64 over tests/chain_check.py's table (precision 1), what each takes to the kernel:
CHAIN = "tests/test_gpu_chain_forward_edges.py"
CHAIN_EDGES = [f"{CHAIN}::test_outputs_match_float64_element_by_element_with_guards",     # every case: outputs element by element, NaN workspace, NaN guard rows
               f"{CHAIN}::test_parameter_gradients_match_float64",                         # every case: the saved activations through the backward pass
               f"{CHAIN}::test_saved_activations_row_by_row",                              # mb 33 / 65 / 1025: act[0..2] one row at a time at the half / workgroup edges
               f"{CHAIN}::test_designed_pre_activations",                                  # pre-activations of exactly 0, -1e-6, -30, -100, -1e4, 8 in every hidden layer
               f"{CHAIN}::test_bit_identical_from_run_to_run"]                             # 17 workgroups twice: the same bits
CHAIN_REPACK = f"{CHAIN}::test_the_forward_follows_an_in_place_parameter_step"             # a forward pass after an in-place parameter change, no refresh()
LOSS = [f"{RL}::test_fused_ppo_loss_matches_autograd", f"{WIDE}::test_ppo_loss_kernel_matches_float64_at_the_games_action_counts", STEP]


def gemm(name, mode):
    """Mangled name of lg::<name><MODE>(lg::GemmArgs); MODE 0 = FWD, 1 = DX, 2 = DW."""
    return f"_ZN2lg{len(name)}{name}ILi{mode}EEEvNS_8GemmArgsE"


def mlp_train(bwd, slots, loss):
    """Mangled name of lg::k_mlp_train<3, 8, 4, 2, BWD, SLOTS, LOSS>(lg::MlpArgs)."""
    return f"_ZN2lg11k_mlp_trainILi3ELi8ELi4ELi2ELb{int(bwd)}ELi{slots}ELb{int(loss)}EEEvNS_7MlpArgsE"


COVERAGE = {
    # forward GEMMs: exact f32 at precision 0 for every shape; the split-bf16 build ONLY where the chain kernel is refused (precision 1:
    # the game shapes, separate 235 / 169 inputs, more than 16 outputs, other hidden widths) -- the generic-path test asserts it is
    gemm("k_gemm_wide", 0): [ROUGH, GENERIC, STEP],
    gemm("k_gemm_wide_bf16x3", 0): [GENERIC, STEP],
    # dX / dW: both builds at the rough widths and at the game shapes (+ the output layer past LG_OUT_MAXN and ragged hidden widths)
    gemm("k_gemm_wide", 1): [ROUGH, GENERIC, STEP],
    gemm("k_gemm_wide", 2): [ROUGH, GENERIC, STEP],
    gemm("k_gemm_wide_bf16x3", 1): [ROUGH, GENERIC, STEP],
    gemm("k_gemm_wide_bf16x3", 2): [ROUGH, GENERIC, STEP],
    "_ZN2lg11k_wide_prepENS_12WidePrepArgsE": [ROUGH, GENERIC, STEP],
    "_ZN2lg13k_wide_reduceENS_14WideReduceArgsE": [ROUGH, GENERIC, STEP],
    "_ZN2lg14k_wide_out_bwdILi16EEEvNS_10OutBwdArgsE": [ROUGH, GENERIC, STEP],
    # chain forward (precision 1, both nets 235 or both 169 wide) and its weight packing; CHAIN_EDGES takes each of <15> and <11> to the
    # ends of its width range and every quad boundary of the last k-step, 1 .. 16 outputs, one net / two nets / two ldx, mb 1 .. 1025
    "_ZN2lg17k_mlp_chain_fwd64ILi15EEEvNS_9ChainArgsE": [ROUGH] + CHAIN_EDGES,
    "_ZN2lg17k_mlp_chain_fwd64ILi11EEEvNS_9ChainArgsE": [ROUGH] + CHAIN_EDGES,
    # ... the packing with them: every width's zeroed columns past in_dim, the biases padded to 32 per tile, and CHAIN_REPACK
    "_ZN2lg12k_chain_packENS_13ChainPackArgsE": [ROUGH] + CHAIN_EDGES + [CHAIN_REPACK],
    # LDS-resident trainer of the 48-128-64-32 networks: forward, backward, backward with the PPO loss inside
    mlp_train(0, 4, 0): [FLAT, RAGGED] + FLAT_FB,
    mlp_train(1, 2, 0): [FLAT, RAGGED] + FLAT_FB,
    mlp_train(1, 2, 1): [MINIBATCH] + FLAT_FUSED,
    "_ZN2lg12k_mlp_reduceENS_13MlpReduceArgsE": [FLAT, RAGGED, MINIBATCH] + FLAT_FB + FLAT_FUSED,
    "k_ppo_loss": LOSS,
}


def kernel_of(symbol):
    """Function name of a symbol in kernel_resources.txt: lg::<name>[<...>] (Itanium: _ZN2lg<len><name>...) or an unmangled name."""
    m = re.match(r"_ZN2lg(\d+)", symbol)
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


def compiled_variants(path=RESOURCES):
    """The learner kernels listed in a kernel_resources.txt."""
    names = set()
    with open(path) as f:
        for line in f:
            m = re.match(r"(\S+)\s", line)
            if m and not line.startswith("#") and kernel_of(m.group(1)) in KERNELS:
                names.add(m.group(1))
    return names


def uncovered(path=RESOURCES):
    return sorted(compiled_variants(path) - set(COVERAGE))


def test_every_learner_kernel_instantiation_has_a_reference_test():
    names = compiled_variants()
    assert {kernel_of(n) for n in names} == set(KERNELS), sorted(names)
    assert uncovered() == [], "instantiations no GPU test compares with a reference: " + ", ".join(uncovered())
    assert set(COVERAGE) == names, "table entries for kernels that are no longer compiled: " + ", ".join(sorted(set(COVERAGE) - names))


def test_every_named_test_function_exists():
    defined = {}
    for tests in COVERAGE.values():
        assert tests
        for t in tests:
            path, func = t.split("::")
            if path not in defined:
                with open(os.path.join(REPO, path)) as f:
                    tree = ast.parse(f.read())
                gpu = any(isinstance(n, ast.Assign) and any(getattr(x, "id", None) == "pytestmark" for x in n.targets)
                          and "gpu" in ast.unparse(n.value) for n in tree.body)
                defined[path] = ({n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}, gpu)
            funcs, gpu = defined[path]
            assert func in funcs, t
            assert gpu, f"{path} is not marked gpu"


def test_a_new_instantiation_is_reported_uncovered(tmp_path):
    extra = [gemm("k_gemm_wide_bf16x3", 3), "_ZN2lg14k_wide_out_bwdILi32EEEvNS_10OutBwdArgsE", mlp_train(1, 4, 1)]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 256  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 1\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
