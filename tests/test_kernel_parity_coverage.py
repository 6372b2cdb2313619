"""Every compiled instantiation of the step kernel (k_step) and of the rigid-body sub-step kernel (k_physics) is compared with the CPU
oracle by at least one GPU test.  csrc/kernel_resources.txt (written by __graft_entry__.build()) lists what hipcc compiled; the table
below names, for each instantiation, the GPU test functions that dispatch it and compare its results with oracle/lg_oracle.c.
A new template instantiation fails this test until a test for it is added to the table.  (CPU only: the modules are parsed, not
imported.)"""
import ast
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")


def k_step(traits, net, hf, pol, nw, sc, roll=False):
    """Mangled name of k_step<Traits, NET, HF, POL, NW, SC, ROLL>(KArgs)."""
    b = lambda x: f"Lb{int(bool(x))}E"
    return f"_Z6k_stepI{len(traits)}{traits}{b(net)}{b(hf)}{b(pol)}Li{nw}E{b(sc)}{b(roll)}Ev5KArgs"


def k_physics(traits, hf, sc):
    """Mangled name of k_physics<Traits, HF, SC>(KArgs, const float *, int)."""
    b = lambda x: f"Lb{int(bool(x))}E"
    return f"_Z9k_physicsI{len(traits)}{traits}{b(hf)}{b(sc)}Ev5KArgsPKfi"


A, C = "AnymalTraits", "CassieTraits"
PARITY, FULL, SELF = "tests/test_gpu_parity.py", "tests/test_gpu_full_size.py", "tests/test_gpu_self_collision.py"
ROLL, VARIANTS = "tests/test_gpu_rollout_oracle.py", "tests/test_gpu_step_variants.py"
A1_VARIANTS = f"{VARIANTS}::test_a1_step_variants_against_the_oracle"       # A1 (PD) x plane / height field x SC x NW 4 / 2 / 1
HF = "tests/test_gpu_hf_contact.py"                                         # designed slopes, risers and map edges, N = 40 (NW = 4)
HF_STEP, HF_SUBSTEP = f"{HF}::test_step_against_the_oracle", f"{HF}::test_substep_against_the_oracle"
FALL = "tests/test_gpu_cassie_fall.py"                                      # Cassie through landing, stance, pelvis contact and the in-step reset
FALL_EVERY, FALL_WAVES = f"{FALL}::test_every_step_of_the_fall_against_the_oracle", f"{FALL}::test_landing_stance_and_fall_with_fewer_helper_waves"
HF_PHYSICS = [HF_SUBSTEP, f"{HF}::test_kernel_force_direction", f"{HF}::test_rotation_equivalence_on_the_device"]

COVERAGE = {
    # quadruped, PD control (a1)
    **{k_step(A, 0, hf, 0, nw, sc): [A1_VARIANTS] + ([HF_STEP] if hf and nw == 4 else []) for hf in (0, 1) for nw in (1, 2, 4) for sc in (0, 1)},
    # quadruped, actuator net, plane (anymal_c_flat: self-collision on; anymal_b: off)
    k_step(A, 1, 0, 0, 4, 0): [f"{PARITY}::test_full_step_parity"],
    k_step(A, 1, 0, 0, 4, 1): [f"{PARITY}::test_full_step_parity", f"{PARITY}::test_tiny_and_ragged_env_counts",
                               f"{SELF}::test_policy_step_parity_with_self_collision"],
    # ... with the actor fused in (lg_step_policy) and T steps per launch (lg_rollout_policy)
    **{k_step(A, 1, 0, 1, 4, sc, roll): [f"{ROLL}::test_rollout_kernel_against_the_oracle_every_step"] for sc in (0, 1) for roll in (0, 1)},
    # quadruped, actuator net, height field (anymal_c_rough)
    k_step(A, 1, 1, 0, 4, 0): [f"{FULL}::test_config3_anymal_rough_4096_full_terrain", f"{FULL}::test_trimesh_vertical_faces_parity", HF_STEP],
    k_step(A, 1, 1, 0, 4, 1): [f"{VARIANTS}::test_anymal_rough_heightfield_with_self_collision", HF_STEP],
    # biped (cassie), PD control
    # (plane: the two tests of test_gpu_parity.py compare the step straight after reset_idx, with the robot in free fall from z = 1; the
    # fall tests are the ones with ground contact -- toes and pelvis -- a terminating env and a reset inside the step)
    k_step(C, 0, 0, 0, 4, 0): [f"{PARITY}::test_full_step_parity", FALL_EVERY],
    k_step(C, 0, 0, 0, 2, 0): [f"{PARITY}::test_step_parity_with_fewer_helper_waves", FALL_WAVES],
    k_step(C, 0, 0, 0, 1, 0): [f"{PARITY}::test_step_parity_with_fewer_helper_waves", FALL_WAVES],
    **{k_step(C, 0, 1, 0, nw, 0): [f"{FULL}::test_cassie_heightfield_step_parity"] + ([HF_STEP, FALL_EVERY] if nw == 4 else []) for nw in (1, 2, 4)},
    # one 5 ms rigid-body sub-step (lg_physics_substep)
    k_physics(A, 0, 0): [f"{PARITY}::test_physics_substep_parity"],
    k_physics(A, 0, 1): [f"{PARITY}::test_physics_substep_parity", f"{SELF}::test_substep_parity_with_crossed_legs"],
    k_physics(A, 1, 0): [f"{FULL}::test_trimesh_vertical_faces_parity"] + HF_PHYSICS,
    k_physics(A, 1, 1): [f"{SELF}::test_substep_parity_with_crossed_legs", HF_SUBSTEP, f"{HF}::test_rotation_equivalence_on_the_device"],
    k_physics(C, 0, 0): [f"{PARITY}::test_physics_substep_parity"],
    k_physics(C, 1, 0): [f"{PARITY}::test_physics_substep_parity", HF_SUBSTEP, f"{HF}::test_rotation_equivalence_on_the_device"],
}


def compiled_variants(path=RESOURCES):
    """The k_step / k_physics kernels listed in a kernel_resources.txt."""
    names = set()
    with open(path) as f:
        for line in f:
            m = re.match(r"(_Z6k_stepI\S+|_Z9k_physicsI\S+)\s", line)
            if m:
                names.add(m.group(1))
    return names


def uncovered(path=RESOURCES):
    return sorted(compiled_variants(path) - set(COVERAGE))


def test_every_step_and_physics_instantiation_has_an_oracle_test():
    names = compiled_variants()
    assert len(names) == 32, len(names)
    assert uncovered() == [], "instantiations no GPU test compares with the oracle: " + ", ".join(uncovered())
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


def test_a_new_variant_is_reported_uncovered(tmp_path):
    extra = k_step(A, 0, 1, 0, 8, 1)
    assert extra not in COVERAGE
    copy = tmp_path / "kernel_resources.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + f"{extra}  VGPRs 256  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 1\n")
    assert uncovered(str(copy)) == [extra]
    assert uncovered() == []
