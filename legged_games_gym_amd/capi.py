"""ctypes mirror of ``include/legged_hip.h`` and the loader of the HIP library.

This is the "thin C-ABI" of the north star: Python hands raw device pointers
(``tensor.data_ptr()``) and plain structs to ``liblegged_hip.so``; it plays
the role ``gymapi``/``gymtorch`` play in the reference (call sites
``legged_gym/envs/base/legged_robot.py:92-96, 111-112, 410-444, 515-529``).

Every entry point of every public header is one row of ``ABI`` (near the end of this file, after the structs it names);
``bind_header`` / ``bind_all`` attach the prototypes and check the struct sizes, ``_call`` is the one return-code check and
``_buffers`` the one cast of a name -> address table into a struct.

There is NO CPU fallback: ``load_library()`` raises if the HIP extension has
not been built (``python -c "import __graft_entry__ as g; g.build()"``).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Dict, Optional

import numpy as np

LG_ABI_VERSION = 22
LG_ADAM_SCRATCH_FLOATS = 2050
LG_MAX_LIMBS, LG_MAX_CHAIN, LG_MAX_DOF = 4, 6, 12
LG_MAX_LIMB_POINTS, LG_MAX_BASE_POINTS, LG_MAX_BODIES = 8, 4, 20
LG_MAX_HEIGHT_POINTS, LG_ACTUATOR_FLOATS = 192, 972

# alphabetical == enum order in legged_hip.h
REWARD_TERMS = ["action_rate", "ang_vel_xy", "base_height", "collision", "dof_acc", "dof_pos_limits",
                "dof_vel", "dof_vel_limits", "feet_air_time", "feet_contact_forces", "lin_vel_z", "no_fly",
                "orientation", "stand_still", "stumble", "termination", "torque_limits", "torques",
                "tracking_ang_vel", "tracking_lin_vel"]
LG_NUM_REWARD_TERMS = len(REWARD_TERMS)
CTRL = {"P": 0, "V": 1, "T": 2, "actuator_net": 3}
TERRAIN_PLANE, TERRAIN_HEIGHTFIELD = 0, 1

f32, i32, u32, u8, i64, u64, i16 = C.c_float, C.c_int32, C.c_uint32, C.c_uint8, C.c_int64, C.c_uint64, C.c_int16


class lg_point(C.Structure):
    _fields_ = [("pos", f32 * 3), ("radius", f32), ("report_body", i32), ("joint", i32)]


class lg_robot_model(C.Structure):
    _fields_ = [
        ("num_limbs", i32), ("chain_len", i32), ("num_bodies", i32), ("_pad0", i32),
        ("base_mass", f32), ("base_com", f32 * 3), ("base_inertia", f32 * 6),
        ("joint_pos", (f32 * 3) * LG_MAX_DOF), ("joint_rot", (f32 * 9) * LG_MAX_DOF), ("joint_axis", (f32 * 3) * LG_MAX_DOF),
        ("body_mass", f32 * LG_MAX_DOF), ("body_com", (f32 * 3) * LG_MAX_DOF), ("body_inertia", (f32 * 6) * LG_MAX_DOF),
        ("dof_lower", f32 * LG_MAX_DOF), ("dof_upper", f32 * LG_MAX_DOF), ("dof_vel_limit", f32 * LG_MAX_DOF),
        ("dof_armature", f32 * LG_MAX_DOF), ("dof_damping", f32 * LG_MAX_DOF),
        ("num_base_points", i32), ("num_limb_points", i32 * LG_MAX_LIMBS), ("_pad1", i32 * 3),
        ("base_points", lg_point * LG_MAX_BASE_POINTS),
        ("limb_points", (lg_point * LG_MAX_LIMB_POINTS) * LG_MAX_LIMBS),
        ("foot_body", i32 * LG_MAX_LIMBS), ("penalised_mask", u32), ("termination_mask", u32),
    ]


class lg_params(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("num_envs", i32), ("decimation", i32), ("control_type", i32),
        ("sim_dt", f32), ("gravity", f32 * 3),
        ("contact_stiffness", f32), ("contact_damping", f32), ("friction_damping", f32), ("contact_margin", f32),
        ("ground_friction", f32), ("limit_stiffness", f32), ("limit_damping", f32), ("stick_velocity", f32),
        ("action_scale", f32), ("clip_actions", f32), ("clip_observations", f32), ("_padf1", f32),
        ("p_gains", f32 * LG_MAX_DOF), ("d_gains", f32 * LG_MAX_DOF), ("default_dof_pos", f32 * LG_MAX_DOF),
        ("torque_limits", f32 * LG_MAX_DOF),
        ("soft_pos_lower", f32 * LG_MAX_DOF), ("soft_pos_upper", f32 * LG_MAX_DOF), ("dof_vel_limits", f32 * LG_MAX_DOF),
        ("soft_dof_vel_limit", f32), ("soft_torque_limit", f32), ("tracking_sigma", f32), ("base_height_target", f32),
        ("max_contact_force", f32), ("dt_policy", f32), ("max_push_vel", f32), ("_padf2", f32),
        ("max_episode_length", i32), ("push_interval", i32), ("resample_interval", i32), ("heading_command", i32),
        ("cmd_lin_vel_x", f32 * 2), ("cmd_lin_vel_y", f32 * 2), ("cmd_ang_vel_yaw", f32 * 2), ("cmd_heading", f32 * 2),
        ("obs_scale_lin_vel", f32), ("obs_scale_ang_vel", f32), ("obs_scale_dof_pos", f32), ("obs_scale_dof_vel", f32),
        ("obs_scale_height", f32),
        ("noise_lin_vel", f32), ("noise_ang_vel", f32), ("noise_gravity", f32), ("noise_dof_pos", f32),
        ("noise_dof_vel", f32), ("noise_height", f32),
        ("add_noise", i32), ("measure_heights", i32), ("num_height_points", i32), ("num_obs", i32),
        ("height_points", (f32 * 2) * LG_MAX_HEIGHT_POINTS),
        ("reward_scale", f32 * LG_NUM_REWARD_TERMS),
        ("only_positive_rewards", i32), ("reward_slot", i32 * LG_NUM_REWARD_TERMS), ("num_reward_slots", i32),
        ("terrain_type", i32), ("hf_rows", i32), ("hf_cols", i32), ("custom_origins", i32),
        ("hf_horizontal_scale", f32), ("hf_vertical_scale", f32), ("hf_border", f32), ("hf_step_threshold", f32),
        ("terrain_curriculum", i32), ("terrain_num_rows", i32), ("terrain_num_cols", i32), ("self_collision", i32),
        ("terrain_env_length", f32), ("max_episode_length_s", f32),
        ("base_init_state", f32 * 13), ("_padf4", f32),
        ("seed", u64),
        # commands.curriculum on the device (legged_hip.h): on/off, tracking_lin_vel's slot, the host rule's constants in double
        ("cmd_curriculum", i32), ("cmd_curriculum_slot", i32), ("cmd_max_curriculum", C.c_double), ("cmd_tracking_scale_dt", C.c_double),
        ("cmd_max_episode_length", C.c_double), ("cmd_episode_length_s", C.c_double),
    ]


_PF, _PU8, _PI64, _PI32, _PI16 = C.POINTER(f32), C.POINTER(u8), C.POINTER(i64), C.POINTER(i32), C.POINTER(i16)


class lg_rollout_buffers(C.Structure):
    """Rollout storage of ``lg_rollout_policy`` (include/legged_hip.h): [steps(+1)][N][...] device arrays owned by the caller."""
    _fields_ = [("steps", i32), ("obs", _PF), ("obs0", _PF), ("actions", _PF), ("mean", _PF), ("rew", _PF), ("dones", _PU8), ("time_outs", _PU8)]


LG_MAX_ROLL_STEPS = 256


class lg_buffers(C.Structure):
    _fields_ = [
        ("root_states", _PF), ("dof_state", _PF), ("contact_forces", _PF), ("obs_buf", _PF), ("rew_buf", _PF),
        ("reset_buf", _PU8), ("time_out_buf", _PU8), ("episode_length_buf", _PI64),
        ("torques", _PF), ("actions", _PF), ("last_actions", _PF), ("last_dof_vel", _PF),
        ("last_root_vel", _PF), ("commands", _PF), ("feet_air_time", _PF), ("last_contacts", _PU8),
        ("base_lin_vel", _PF), ("base_ang_vel", _PF), ("projected_gravity", _PF),
        ("measured_heights", _PF), ("sea_hidden_state", _PF), ("sea_cell_state", _PF),
        ("episode_sums", _PF), ("episode_means", _PF), ("extras_accum", _PF), ("step_counter", _PI64), ("env_origins", _PF),
        ("terrain_levels", _PI32), ("terrain_types", _PI32), ("terrain_origins", _PF),
        ("height_samples", _PI16), ("friction_coeffs", _PF), ("base_mass_delta", _PF), ("cmd_range", C.POINTER(C.c_double)),
    ]


BUFFER_FIELDS = [name for name, _ in lg_buffers._fields_]


# ----------------------------------------------------------------------------- packing
def _fill(dst, src):
    flat = np.ascontiguousarray(np.asarray(src, dtype=np.float64).ravel(), dtype=np.float32)   # keep alive during memmove
    if 4 * flat.size > C.sizeof(dst):
        raise ValueError("source larger than the destination field")
    C.memmove(dst, flat.ctypes.data, 4 * flat.size)


def _sym6(I):
    I = np.asarray(I)
    return [I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]


def pack_model(model, foot_name: str, penalize_on, terminate_on, armature: float = 0.0) -> lg_robot_model:
    """``RobotModel`` (model compiler) -> ``lg_robot_model``; the body lookups by
    substring mirror legged_robot.py:696-702."""
    K, L, n = model.num_limbs, model.chain_len, model.num_dof
    if K * L != LG_MAX_DOF or K > LG_MAX_LIMBS or L > LG_MAX_CHAIN:
        raise ValueError(f"robot must be K limbs x L joints with K*L == 12, got K={K} L={L}")
    if model.num_bodies > LG_MAX_BODIES:
        raise ValueError("too many report bodies")
    m = lg_robot_model()
    m.num_limbs, m.chain_len, m.num_bodies = K, L, model.num_bodies
    m.base_mass = model.base_mass
    _fill(m.base_com, model.base_com)
    _fill(m.base_inertia, _sym6(model.base_inertia))
    _fill(m.joint_pos, model.joint_pos)
    _fill(m.joint_rot, model.joint_rot)
    _fill(m.joint_axis, model.joint_axis)
    _fill(m.body_mass, model.body_mass)
    _fill(m.body_com, model.body_com)
    _fill(m.body_inertia, [_sym6(I) for I in model.body_inertia])
    lo = np.where(model.dof_has_limits, model.dof_lower, 1.0)
    hi = np.where(model.dof_has_limits, model.dof_upper, -1.0)     # lower > upper encodes "no limit"
    _fill(m.dof_lower, lo)
    _fill(m.dof_upper, hi)
    _fill(m.dof_vel_limit, model.dof_velocity)
    _fill(m.dof_armature, np.full(n, armature))
    _fill(m.dof_damping, model.dof_damping)

    def put(dst, cp, joint):
        _fill(dst.pos, cp.pos)
        dst.radius, dst.report_body, dst.joint = cp.radius, cp.report_body, joint

    if len(model.base_points) > LG_MAX_BASE_POINTS:
        raise ValueError("too many base collision points")
    m.num_base_points = len(model.base_points)
    for i, cp in enumerate(model.base_points):
        put(m.base_points[i], cp, -1)
    for k in range(K):
        pts = model.limb_points[k]
        if len(pts) > LG_MAX_LIMB_POINTS:
            raise ValueError("too many limb collision points")
        m.num_limb_points[k] = len(pts)
        for i, cp in enumerate(pts):
            put(m.limb_points[k][i], cp, model.limb_point_joint[k][i])
    feet = model.bodies_matching(foot_name)
    if len(feet) != K:
        raise ValueError(f"expected one foot body per limb, found {len(feet)} for {foot_name!r}")
    for k, b in enumerate(feet):
        dyn = model.report_parent_dyn[b]
        if not (1 + k * L <= dyn <= (k + 1) * L):
            raise ValueError("foot bodies must be ordered like the limbs")
        m.foot_body[k] = b
    pen = sorted({b for s in penalize_on for b in model.bodies_matching(s)})
    ter = sorted({b for s in terminate_on for b in model.bodies_matching(s)})
    m.penalised_mask = sum(1 << b for b in pen)
    m.termination_mask = sum(1 << b for b in ter)
    return m


class lg_mlp_net(C.Structure):
    """include/legged_hip.h: lg_mlp_net (device pointers as integers)."""
    _fields_ = [("weights", C.c_void_p * 4), ("biases", C.c_void_p * 4), ("grad_weights", C.c_void_p * 4), ("grad_biases", C.c_void_p * 4),
                ("input", C.c_void_p), ("output", C.c_void_p), ("grad_output", C.c_void_p), ("dims", i32 * 5)]


class lg_ppo_batch(C.Structure):
    """include/legged_hip.h: lg_ppo_batch."""
    _fields_ = [(n, C.c_void_p) for n in ("actions", "old_log_prob", "old_mu", "old_sigma", "advantages", "old_values", "returns", "std")] + \
               [("clip", C.c_float), ("value_coef", C.c_float), ("entropy_coef", C.c_float), ("use_clipped_value", i32),
                ("d_std", C.c_void_p), ("stats", C.c_void_p), ("loss_acc", C.c_void_p)]


class lg_rollout_step(C.Structure):
    """include/legged_hip.h: lg_rollout_step."""
    _fields_ = [(n, C.c_void_p) for n in ("obs", "actions", "mean", "rewards", "dones", "time_outs", "storage_obs", "storage_actions",
                                          "storage_mu", "storage_rewards", "storage_dones", "storage_time_outs", "cur_return", "cur_length",
                                          "sums", "std", "storage_sigma", "storage_log_prob")] + [("num_envs", i32), ("num_obs", i32), ("num_actions", i32)]


class lg_rollout_post(C.Structure):
    """include/legged_hip.h: lg_rollout_post."""
    _fields_ = [(n, C.c_void_p) for n in ("actions", "mean", "rewards", "dones", "time_outs", "std", "sigma", "log_prob", "time_outs_f",
                                          "cur_return", "cur_length", "sums")] + [("steps", i32), ("num_envs", i32), ("num_actions", i32)]


class lg_adam_tensor(C.Structure):
    """include/legged_hip.h: lg_adam_tensor."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_void_p),
                ("numel", i64)]


def struct_to_dict(s) -> Dict:
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        out[name] = np.ctypeslib.as_array(v).copy() if hasattr(v, "_length_") else v
    return out


# ----------------------------------------------------------------------------- library
class Library:
    """One shared library of csrc/: its file, the environment variable that selects another build of the same sources, its entry points
    (name -> (argtypes, restype)), the module attribute that caches the loaded handle (``handle`` reads and writes it), optionally the
    ``sizeof`` entry point and the structs it sizes by index, and what loading it gives.  ``bind_hook`` / ``check`` replace the plain
    binding / follow it (the main library's per-header tables and ABI version)."""

    def __init__(self, file, env, abi, cache, sizeof=None, what="", bind_hook=None, check=None):
        self.file, self.env, self.abi, self.sizeof, self.what, self.bind_hook, self.check = file, env, abi, sizeof, what, bind_hook, check
        self.cache = cache                 # the module attribute that holds the loaded handle (``_gru_lib`` ...): callers that reset it still do
        globals()[cache] = None

    @property
    def handle(self):
        return globals()[self.cache]

    @handle.setter
    def handle(self, lib):
        globals()[self.cache] = lib


LIBRARIES: Dict[str, Library] = {}       # "main" and the eight side libraries, each registered where its ABI is declared


def path(name: str) -> str:
    """The library's in-tree file, or what its environment variable names (another build of the same sources)."""
    rec = LIBRARIES[name]
    return os.environ.get(rec.env) or os.path.join(os.path.dirname(os.path.realpath(__file__)), "csrc", rec.file)


def bind(name: str, lib):
    """Attach argtypes/restype for the library's entry points and check the layouts of the structs its ``sizeof`` sizes."""
    rec = LIBRARIES[name]
    if rec.bind_hook is not None:
        return rec.bind_hook(lib)
    for symbol, (argtypes, restype) in rec.abi.items():
        fn = getattr(lib, symbol)
        fn.argtypes, fn.restype = argtypes, restype
    if rec.sizeof is not None:
        sizeof, structs = rec.sizeof
        for which, st in structs.items():
            size = getattr(lib, sizeof)(which)
            if size != C.sizeof(st):
                raise RuntimeError(f"struct layout mismatch for {st.__name__}: C {size} vs ctypes {C.sizeof(st)}")
    return lib


def load(name: str, file: Optional[str] = None):
    """Load the library (from ``file``, default ``path(name)``) or fail loudly -- never a CPU substitute."""
    rec = LIBRARIES[name]
    if rec.handle is not None:
        return rec.handle
    file = file or path(name)
    if not os.path.isfile(file):
        raise RuntimeError(
            f"HIP extension {file} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    rec.handle = bind(name, C.CDLL(file))
    if rec.check is not None:
        rec.check(rec.handle)
    return rec.handle


def _library_names(name: str):
    """The three public names of a library: ``*_library_path()``, ``bind_*(lib)``, ``load_*_library()``."""
    return functools.partial(path, name), functools.partial(bind, name), functools.partial(load, name)


def library_path() -> str:
    """In-tree liblegged_hip.so; LG_HIP_LIB selects another build of the same sources (tools/profile_sections.py)."""
    return path("main")


def load_library():
    """Load the HIP extension (from ``library_path()``) or fail loudly -- never a CPU substitute."""
    return load("main", library_path())


def _call(name, *args, ok=(0,)):
    """Call entry point ``name`` of the library; its return code if that is in ``ok``, otherwise a RuntimeError with ``lg_last_error``."""
    lib = load_library()
    rc = getattr(lib, name)(*args)
    if rc not in ok:
        raise RuntimeError(f"{name} failed ({rc}): {lib.lg_last_error().decode()}")
    return rc


def _buffers(struct_type, pointers: Dict[str, int], fields=None):
    """``struct_type`` with its pointer ``fields`` (default: every field) cast from a name -> address table; missing names stay null."""
    b = struct_type()
    for name, ctype in struct_type._fields_:
        if fields is None or name in fields:
            setattr(b, name, C.cast(C.c_void_p(pointers.get(name, 0) or 0), ctype))
    return b


# ----------------------------------------------------------------------------- game layer (include/legged_game.h)
LG_GAME_NUM_OBS, LG_GAME_NUM_ACTIONS = 19, 6


class lg_game_params(C.Structure):
    """include/legged_game.h: lg_game_params (passed by value in the kernel arguments)."""
    _fields_ = [
        ("num_envs", i32), ("decimation", i32), ("heading_command", i32), ("only_positive_rewards", i32),
        ("custom_origins", i32), ("_pad0", i32), ("seed", u64),
        ("cmd_lin_vel_x", f32 * 2), ("cmd_lin_vel_y", f32 * 2), ("predator_lin_vel_x", f32 * 2), ("predator_lin_vel_y", f32 * 2),
        ("capture_dist", f32), ("env_radius", f32), ("half_fov", f32), ("max_rel_pos", f32),
        ("ll_rew_weight", f32), ("scale_evasion_dt", f32), ("scale_pursuit_dt", f32), ("sim_dt", f32),
        ("predator_z", f32), ("_pad1", f32), ("base_init_state", f32 * 13), ("_pad2", f32),
    ]


class lg_game_buffers(C.Structure):
    """include/legged_game.h: lg_game_buffers (raw device pointers)."""
    _fields_ = [
        ("command", _PF), ("ll_root_states", _PF), ("ll_commands", _PF), ("ll_env_origins", _PF), ("ll_rew_buf", _PF),
        ("ll_reset_buf", _PU8), ("ll_step_counter", _PI64),
        ("predator_pos", _PF), ("obs", _PF), ("rew", _PF), ("reset_buf", _PU8), ("curr_episode_step", _PI64),
        ("episode_length_buf", _PI64), ("episode_sums", _PF),
    ]


GAME_BUFFER_FIELDS = [name for name, _ in lg_game_buffers._fields_]


def game_buffers(pointers: Dict[str, int]) -> lg_game_buffers:
    """``lg_game_buffers`` from a name -> device address table (missing names stay null)."""
    return _buffers(lg_game_buffers, pointers)


def game_pre(params: lg_game_params, buffers: lg_game_buffers, stream: int = 0):
    _call("lg_game_pre", C.byref(params), C.byref(buffers), stream)


def game_act(hl_policy, ll_policy, params: lg_game_params, buffers: lg_game_buffers, hl_obs: int, ll_obs: int, ll_actions: int, mean: int, seed: int,
             step: int, step_counter: Optional[int], deterministic: bool, sample: Optional[int] = None, sigma: Optional[int] = None,
             log_prob: Optional[int] = None, obs_copy: Optional[int] = None, stream: int = 0) -> int:
    """``lg_game_act``: both actors of a high-level step and the command clip in one launch.  Returns 0, or -4 when the actor pair /
    wide precision has no shared kernel (the caller then issues ``lg_policy_act`` x 2 + ``lg_game_pre``); raises on any other error."""
    return _call("lg_game_act", hl_policy, ll_policy, C.byref(params), C.byref(buffers), hl_obs, ll_obs, ll_actions, mean, int(seed), int(step), step_counter,
                 int(bool(deterministic)), sample, sigma, log_prob, obs_copy, stream, ok=(0, -4))


def game_post(params: lg_game_params, buffers: lg_game_buffers, common_step_counter: int, stream: int = 0):
    _call("lg_game_post", C.byref(params), C.byref(buffers), int(common_step_counter), stream)


# ----------------------------------------------------------------------------- decentralised game (include/legged_dec_game.h)
LG_DEC_NUM_OBS_PREY, LG_DEC_NUM_OBS_PRED, LG_DEC_NUM_ACTIONS_PREY, LG_DEC_NUM_ACTIONS_PRED, LG_DEC_NUM_SUMS = 16, 3, 4, 2, 3
_PU32 = C.POINTER(u32)


class lg_dec_game_params(C.Structure):
    """include/legged_dec_game.h: lg_dec_game_params (passed by value in the kernel arguments)."""
    _fields_ = [
        ("num_envs", i32), ("decimation", i32), ("heading_command", i32), ("custom_origins", i32),
        ("only_positive_rewards_prey", i32), ("only_positive_rewards_pred", i32), ("max_episode_length", i32), ("_pad0", i32), ("seed", u64),
        ("cmd_lin_vel_x", f32 * 2), ("cmd_lin_vel_y", f32 * 2), ("predator_lin_vel_x", f32 * 2), ("predator_lin_vel_y", f32 * 2),
        ("capture_dist", f32), ("half_fov", f32), ("max_rel_pos", f32), ("ll_rew_weight", f32),
        ("scale_evasion_dt", f32), ("scale_pursuit_dt", f32), ("scale_termination_prey_dt", f32), ("sim_dt", f32),
        ("predator_z", f32), ("max_episode_length_s", f32), ("base_init_state", f32 * 13), ("_pad1", f32), ("default_dof_pos", f32 * LG_MAX_DOF),
    ]


class lg_dec_game_buffers(C.Structure):
    """include/legged_dec_game.h: lg_dec_game_buffers (raw device pointers)."""
    _fields_ = [
        ("command_prey", _PF), ("command_pred", _PF), ("ll_root_states", _PF), ("ll_dof_state", _PF), ("ll_commands", _PF), ("ll_env_origins", _PF),
        ("ll_rew_buf", _PF), ("ll_reset_buf", _PU8), ("ll_step_counter", _PI64),
        ("predator_pos", _PF), ("obs_prey", _PF), ("obs_pred", _PF), ("rew_prey", _PF), ("rew_pred", _PF), ("reset_buf", _PU8), ("time_out_buf", _PU8),
        ("curr_episode_step", _PI64), ("episode_length_buf", _PI64), ("episode_sums", _PF), ("episode_means", _PF), ("extras_accum", _PF),
        ("extras_ticket", _PU32),
    ]


DEC_GAME_BUFFER_FIELDS = [name for name, _ in lg_dec_game_buffers._fields_]


class lg_dec_act_outputs(C.Structure):
    """include/legged_dec_game.h: lg_dec_act_outputs (optional per-agent outputs of lg_dec_game_act; device addresses or None)."""
    _fields_ = [("sample", C.c_void_p), ("sigma", C.c_void_p), ("log_prob", C.c_void_p), ("obs_copy", C.c_void_p)]


def dec_game_buffers(pointers: Dict[str, int]) -> lg_dec_game_buffers:
    """``lg_dec_game_buffers`` from a name -> device address table (missing names stay null)."""
    return _buffers(lg_dec_game_buffers, pointers)


def dec_game_pre(params: lg_dec_game_params, buffers: lg_dec_game_buffers, stream: int = 0):
    _call("lg_dec_game_pre", C.byref(params), C.byref(buffers), stream)


def dec_game_act(pred_policy, prey_policy, ll_policy, params: lg_dec_game_params, buffers: lg_dec_game_buffers, pred_obs: int, prey_obs: int, ll_obs: int,
                 ll_actions: int, mean_pred: int, mean_prey: int, seed_pred: int, seed_prey: int, step: int, step_counter: Optional[int],
                 deterministic_pred: bool, deterministic_prey: bool, out_pred: Optional[lg_dec_act_outputs] = None,
                 out_prey: Optional[lg_dec_act_outputs] = None, stream: int = 0) -> int:
    """``lg_dec_game_act``: the three actors of a step and the command clips in one launch.  Returns 0, or -4 when the actor triple / wide
    precision has no shared kernel (the caller then issues ``lg_policy_act`` x 3 + ``lg_dec_game_pre``); raises on any other error."""
    return _call("lg_dec_game_act", pred_policy, prey_policy, ll_policy, C.byref(params), C.byref(buffers), pred_obs, prey_obs, ll_obs, ll_actions, mean_pred, mean_prey,
                 int(seed_pred), int(seed_prey), int(step), step_counter, int(bool(deterministic_pred)), int(bool(deterministic_prey)),
                 C.byref(out_pred) if out_pred is not None else None, C.byref(out_prey) if out_prey is not None else None, stream, ok=(0, -4))


def dec_game_post(params: lg_dec_game_params, buffers: lg_dec_game_buffers, common_step_counter: int, stream: int = 0):
    _call("lg_dec_game_post", C.byref(params), C.byref(buffers), int(common_step_counter), stream)


# ----------------------------------------------------------------------------- scripted pursuer (include/legged_pursuer_game.h)
class lg_pursuer_params(C.Structure):
    """include/legged_pursuer_game.h: lg_pursuer_params (passed by value in the kernel arguments)."""
    _fields_ = [("max_lin_vel", f32), ("min_lin_vel", f32), ("gain", f32), ("max_episode_length", i32)]


def pursuer_post(params: lg_game_params, pursuer: lg_pursuer_params, buffers: lg_game_buffers, predator_command: Optional[int],
                 common_step_counter: int, stream: int = 0):
    """``lg_pursuer_post``: ``lg_game_post`` with the scripted pursuer's velocity, which it writes to ``predator_command`` [N,2] (or None)."""
    _call("lg_pursuer_post", C.byref(params), C.byref(pursuer), C.byref(buffers), predator_command, int(common_step_counter), stream)


# ----------------------------------------------------------------------------- game outcome statistics (include/legged_game_outcome.h)
LG_OUTCOME_NUM_COUNTS, LG_OUTCOME_NUM_MEANS = 7, 6
OUTCOME_COUNTS = ("episodes", "captured", "prey_out", "predator_out", "fell", "survived", "steps")     # the order of accum / totals
OUTCOME_MEANS = OUTCOME_COUNTS[1:]                                                                    # the order of means: five rates, mean steps


class lg_outcome_buffers(C.Structure):
    """include/legged_game_outcome.h: lg_outcome_buffers (raw device pointers)."""
    _fields_ = [("ll_time_out_buf", _PU8), ("accum", C.POINTER(u64)), ("ticket", C.POINTER(C.c_uint32)), ("means", _PF), ("totals", C.POINTER(u64))]


OUTCOME_BUFFER_FIELDS = [name for name, _ in lg_outcome_buffers._fields_]


def outcome_buffers(pointers: Dict[str, int]) -> lg_outcome_buffers:
    """``lg_outcome_buffers`` from a name -> device address table (missing names stay null)."""
    return _buffers(lg_outcome_buffers, pointers)


def outcome_post(params: lg_game_params, buffers: lg_game_buffers, outcome: lg_outcome_buffers, common_step_counter: int, stream: int = 0):
    """``lg_outcome_post``: ``lg_game_post`` that also counts why the done envs' episodes ended."""
    _call("lg_outcome_post", C.byref(params), C.byref(buffers), C.byref(outcome), int(common_step_counter), stream)


def outcome_pursuer_post(params: lg_game_params, pursuer: lg_pursuer_params, buffers: lg_game_buffers, outcome: lg_outcome_buffers,
                         predator_command: Optional[int], common_step_counter: int, stream: int = 0):
    """``lg_outcome_pursuer_post``: ``lg_pursuer_post`` that also counts why the done envs' episodes ended."""
    _call("lg_outcome_pursuer_post", C.byref(params), C.byref(pursuer), C.byref(buffers), C.byref(outcome), predator_command,
          int(common_step_counter), stream)


# ----------------------------------------------------------------------------- decentralised game's outcome statistics (include/legged_dec_game_outcome.h)
LG_DEC_OUTCOME_NUM_COUNTS, LG_DEC_OUTCOME_NUM_MEANS = 6, 5
DEC_OUTCOME_COUNTS = ("episodes", "captured", "timed_out", "fell", "ll_timed_out", "steps")     # the order of accum / totals
DEC_OUTCOME_MEANS = DEC_OUTCOME_COUNTS[1:]                                                      # the order of means: four rates, mean steps


class lg_dec_outcome_buffers(C.Structure):
    """include/legged_dec_game_outcome.h: lg_dec_outcome_buffers (raw device pointers)."""
    _fields_ = [("ll_time_out_buf", _PU8), ("accum", C.POINTER(u64)), ("means", _PF), ("totals", C.POINTER(u64))]


DEC_OUTCOME_BUFFER_FIELDS = [name for name, _ in lg_dec_outcome_buffers._fields_]


def dec_outcome_buffers(pointers: Dict[str, int]) -> lg_dec_outcome_buffers:
    """``lg_dec_outcome_buffers`` from a name -> device address table (missing names stay null)."""
    return _buffers(lg_dec_outcome_buffers, pointers)


def dec_outcome_post(params: lg_dec_game_params, buffers: lg_dec_game_buffers, outcome: lg_dec_outcome_buffers, common_step_counter: int, stream: int = 0):
    """``lg_dec_outcome_post``: ``lg_dec_game_post`` that also counts why the done envs' episodes ended."""
    _call("lg_dec_outcome_post", C.byref(params), C.byref(buffers), C.byref(outcome), int(common_step_counter), stream)


# ----------------------------------------------------------------------------- decentralised game's opponent pool (include/legged_dec_game_pool.h)
LG_DEC_POOL_MAX, LG_DEC_POOL_BLOCK_ENVS = 16, 32
DEC_POOL_ROLES = {"prey": 1, "pred": 2}


class lg_dec_pool_info(C.Structure):
    """include/legged_dec_game_pool.h: lg_dec_pool_info (what ``lg_dec_pool_query`` reports)."""
    _fields_ = [("count", i32), ("role", i32), ("device", i32), ("_pad", i32), ("table", C.c_void_p)]


def dec_pool_create(member_handles, role: str, device: int = 0) -> C.c_void_p:
    """``lg_dec_pool_create`` over ``lg_policy`` handles (``FusedActor.handle``); ``role`` is "prey" or "pred".  The handles must outlive the
    pool and must not be re-created (``FusedActor.sync`` does; ``sync_device`` repacks in place, which the pool follows)."""
    handles = (C.c_void_p * len(member_handles))(*[h.value if isinstance(h, C.c_void_p) else h for h in member_handles])
    out = C.c_void_p()
    _call("lg_dec_pool_create", handles, len(member_handles), DEC_POOL_ROLES[role], int(device), C.byref(out))
    return out


def dec_pool_destroy(pool):
    if pool:
        load_library().lg_dec_pool_destroy(pool)


def dec_pool_query(pool) -> lg_dec_pool_info:
    info = lg_dec_pool_info()
    _call("lg_dec_pool_query", pool, C.byref(info))
    return info


def dec_pool_act(pred_policy, prey_policy, ll_policy, pool_pred, block_slot_pred: Optional[int], pool_prey, block_slot_prey: Optional[int],
                 params: lg_dec_game_params, buffers: lg_dec_game_buffers, pred_obs: int, prey_obs: int, ll_obs: int, ll_actions: int, mean_pred: int,
                 mean_prey: int, seed_pred: int, seed_prey: int, step: int, step_counter: Optional[int], deterministic_pred: bool, deterministic_prey: bool,
                 out_pred: Optional[lg_dec_act_outputs] = None, out_prey: Optional[lg_dec_act_outputs] = None, stream: int = 0) -> int:
    """``lg_dec_pool_act``: ``lg_dec_game_act`` with the weights of a pooled role chosen per 32-env block.  ``pool_*``: a pool handle or None,
    ``block_slot_*``: the device address of its int32 slot table.  Returns 0, or -4 when there is no shared kernel for the wide precision /
    the shapes (the caller then issues ``lg_policy_act`` per member + ``lg_dec_game_pre``); raises on any other error."""
    return _call("lg_dec_pool_act", pred_policy, prey_policy, ll_policy, pool_pred, block_slot_pred, pool_prey, block_slot_prey, C.byref(params), C.byref(buffers),
                 pred_obs, prey_obs, ll_obs, ll_actions, mean_pred, mean_prey, int(seed_pred), int(seed_prey), int(step), step_counter,
                 int(bool(deterministic_pred)), int(bool(deterministic_prey)), C.byref(out_pred) if out_pred is not None else None,
                 C.byref(out_prey) if out_prey is not None else None, stream, ok=(0, -4))


# ----------------------------------------------------------------------------- outcome statistics per pool member (include/legged_dec_game_member_outcome.h)
LG_DEC_MEMBER_OUTCOME_ROWS = LG_DEC_POOL_MAX


class lg_dec_member_outcome_buffers(C.Structure):
    """include/legged_dec_game_member_outcome.h: lg_dec_member_outcome_buffers (raw device pointers and the pool's member count)."""
    _fields_ = [("block_slot", C.POINTER(i32)), ("member_accum", C.POINTER(u64)), ("member_totals", C.POINTER(u64)), ("count", i32), ("_pad", i32)]


DEC_MEMBER_OUTCOME_BUFFER_FIELDS = ["block_slot", "member_accum", "member_totals"]       # the pointers


def dec_member_outcome_buffers(pointers: Dict[str, int], count: int) -> lg_dec_member_outcome_buffers:
    """``lg_dec_member_outcome_buffers`` from a name -> device address table (missing names stay null) and the pool's member count."""
    b = _buffers(lg_dec_member_outcome_buffers, pointers, DEC_MEMBER_OUTCOME_BUFFER_FIELDS)
    b.count = int(count)
    return b


def dec_member_outcome_post(params: lg_dec_game_params, buffers: lg_dec_game_buffers, outcome: lg_dec_outcome_buffers, members: lg_dec_member_outcome_buffers,
                            common_step_counter: int, stream: int = 0):
    """``lg_dec_member_outcome_post``: ``lg_dec_outcome_post`` that also keeps the six counts per opponent-pool member."""
    _call("lg_dec_member_outcome_post", C.byref(params), C.byref(buffers), C.byref(outcome), C.byref(members), int(common_step_counter), stream)


# ---------------------------------------------------------------------------------------------------------------- legged_recurrent.h
LG_LSTM_MAX_IN, LG_LSTM_MAX_HIDDEN, LG_LSTM_BLOCK_ENVS = 256, 256, 32


def lstm_supported(num_in: int, hidden: int) -> bool:
    """The shapes ``lg_lstm_create`` takes."""
    return 1 <= num_in <= LG_LSTM_MAX_IN and 32 <= hidden <= LG_LSTM_MAX_HIDDEN and hidden % 32 == 0


# ----------------------------------------------------------------------------- the ABI: every entry point of every header
_vp, _P, _int = C.c_void_p, C.POINTER, C.c_int
_SIZEOF = ([_int], _int)
_DEC_ACT_TAIL = [_P(lg_dec_game_params), _P(lg_dec_game_buffers), _vp, _vp, _vp, _vp, _vp, _vp, u64, u64, i64, _vp, i32, i32,
                 _P(lg_dec_act_outputs), _P(lg_dec_act_outputs), _vp]
# header -> ({symbol: (argtypes, restype)} in the header's order, its *_sizeof function or None, the structs that function sizes by index)
ABI = {
    "legged_hip.h": ({
        "lg_create": ([_P(lg_params), _P(lg_robot_model), _PF, _int, _P(_vp)], _int),
        "lg_destroy": ([_vp], None),
        "lg_bind": ([_vp, _P(lg_buffers)], _int),
        "lg_step": ([_vp, _vp, i64, _vp], _int),
        "lg_set_deferred_extras": ([_vp, i32], _int),
        "lg_extras_flush": ([_vp, i64, _vp], _int),
        "lg_reset_idx": ([_vp, _vp, i32, i64, _vp], _int),
        "lg_actuator_forward": ([_vp, _vp, _vp, _vp, _vp, _vp, i32, _vp], _int),
        "lg_physics_substep": ([_vp, _vp, i32, _vp], _int),
        "lg_compute_observations_only": ([_vp, i64, _vp], _int),
        "lg_resample_reset_commands": ([_vp, i64, _vp], _int),
        "lg_set_obs_buffer": ([_vp, _vp], _int),
        "lg_set_params": ([_vp, _P(lg_params)], _int),
        "lg_policy_create": ([_P(i32), _P(_PF), _P(_PF), _PF, _int, _P(_vp)], _int),
        "lg_policy_destroy": ([_vp], None),
        "lg_policy_act": ([_vp, _vp, _vp, _vp, i32, u64, i64, _vp, i32, _vp], _int),
        "lg_policy_load_device": ([_vp, _vp, _vp, _vp, _vp], _int),
        "lg_step_policy": ([_vp, _vp, _vp, _vp, _vp, u64, i32, i64, _vp], _int),
        "lg_rollout_policy": ([_vp, _vp, _P(lg_rollout_buffers), u64, i32, i64, _vp], _int),
        "lg_gae_returns": ([_vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, i32, i32, _vp], _int),
        "lg_mlp_forward": ([_P(lg_mlp_net), i32, _vp, i32, _vp], _int),
        "lg_mlp_workspace_bytes": ([_P(lg_mlp_net), i32], C.c_size_t),
        "lg_mlp_backward": ([_P(lg_mlp_net), i32, _vp, i32, _vp, C.c_size_t, _vp], _int),
        "lg_mlp_wide_workspace_bytes": ([_P(lg_mlp_net), i32, i32], C.c_size_t),
        "lg_mlp_wide_set_precision": ([_int], _int),
        "lg_mlp_wide_forward": ([_P(lg_mlp_net), i32, _vp, i32, _vp, C.c_size_t, _vp], _int),
        "lg_mlp_wide_backward": ([_P(lg_mlp_net), i32, _vp, i32, _vp, C.c_size_t, _vp], _int),
        "lg_ppo_minibatch": ([_P(lg_mlp_net), _vp, i32, _P(lg_ppo_batch), _vp, C.c_size_t, _vp], _int),
        "lg_mlp_trace": ([_vp], None),
        "lg_rollout_record": ([_P(lg_rollout_step), _vp], _int),
        "lg_rollout_finish": ([_P(lg_rollout_post), _vp], _int),
        "lg_adam_step": ([_P(lg_adam_tensor), i32, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _vp, C.c_float, _vp, _vp], _int),
        "lg_ppo_loss": ([_vp] * 11 + [C.c_float, C.c_float, C.c_float, i32, _vp, _vp, _vp, _vp, i32, i32, _vp], _int),
        "lg_device_status": ([_vp, i32], _int),
        "lg_clear_device_status": ([_vp], _int),
        "lg_debug_handover": ([_vp, i32, i32], _int),
        "lg_last_error": ([], C.c_char_p),
        "lg_abi_version": ([], _int),
        "lg_sizeof": _SIZEOF,
    }, "lg_sizeof", (lg_params, lg_robot_model, lg_buffers, lg_point, lg_mlp_net, lg_adam_tensor, lg_rollout_step, lg_ppo_batch)),
    "legged_game.h": ({
        "lg_game_pre": ([_P(lg_game_params), _P(lg_game_buffers), _vp], _int),
        "lg_game_post": ([_P(lg_game_params), _P(lg_game_buffers), i64, _vp], _int),
        "lg_game_act": ([_vp, _vp, _P(lg_game_params), _P(lg_game_buffers), _vp, _vp, _vp, _vp, u64, i64, _vp, i32, _vp, _vp, _vp, _vp, _vp], _int),
        "lg_game_sizeof": _SIZEOF,
    }, "lg_game_sizeof", (lg_game_params, lg_game_buffers)),
    "legged_dec_game.h": ({
        "lg_dec_game_pre": ([_P(lg_dec_game_params), _P(lg_dec_game_buffers), _vp], _int),
        "lg_dec_game_post": ([_P(lg_dec_game_params), _P(lg_dec_game_buffers), i64, _vp], _int),
        "lg_dec_game_act": ([_vp, _vp, _vp] + _DEC_ACT_TAIL, _int),
        "lg_dec_game_sizeof": _SIZEOF,
    }, "lg_dec_game_sizeof", (lg_dec_game_params, lg_dec_game_buffers, lg_dec_act_outputs)),
    "legged_pursuer_game.h": ({
        "lg_pursuer_post": ([_P(lg_game_params), _P(lg_pursuer_params), _P(lg_game_buffers), _vp, i64, _vp], _int),
        "lg_pursuer_sizeof": _SIZEOF,
    }, "lg_pursuer_sizeof", (lg_pursuer_params,)),
    "legged_game_outcome.h": ({
        "lg_outcome_post": ([_P(lg_game_params), _P(lg_game_buffers), _P(lg_outcome_buffers), i64, _vp], _int),
        "lg_outcome_pursuer_post": ([_P(lg_game_params), _P(lg_pursuer_params), _P(lg_game_buffers), _P(lg_outcome_buffers), _vp, i64, _vp], _int),
        "lg_outcome_sizeof": _SIZEOF,
    }, "lg_outcome_sizeof", (lg_outcome_buffers,)),
    "legged_dec_game_outcome.h": ({
        "lg_dec_outcome_post": ([_P(lg_dec_game_params), _P(lg_dec_game_buffers), _P(lg_dec_outcome_buffers), i64, _vp], _int),
        "lg_dec_outcome_sizeof": _SIZEOF,
    }, "lg_dec_outcome_sizeof", (lg_dec_outcome_buffers,)),
    "legged_dec_game_pool.h": ({
        "lg_dec_pool_create": ([_P(_vp), i32, i32, i32, _P(_vp)], _int),
        "lg_dec_pool_destroy": ([_vp], _int),
        "lg_dec_pool_query": ([_vp, _P(lg_dec_pool_info)], _int),
        "lg_dec_pool_act": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp] + _DEC_ACT_TAIL, _int),
        "lg_dec_pool_sizeof": _SIZEOF,
    }, "lg_dec_pool_sizeof", (lg_dec_pool_info,)),
    "legged_dec_game_member_outcome.h": ({
        "lg_dec_member_outcome_post": ([_P(lg_dec_game_params), _P(lg_dec_game_buffers), _P(lg_dec_outcome_buffers), _P(lg_dec_member_outcome_buffers), i64, _vp], _int),
        "lg_dec_member_outcome_sizeof": _SIZEOF,
    }, "lg_dec_member_outcome_sizeof", (lg_dec_member_outcome_buffers,)),
    "legged_recurrent.h": ({
        "lg_lstm_create": ([i32, i32, _vp, _vp, _vp, _vp, i32, _P(_vp)], _int),
        "lg_lstm_load_device": ([_vp, _vp, _vp, _vp, _vp, _vp], _int),
        "lg_lstm_destroy": ([_vp], _int),
        "lg_lstm_step": ([_vp] * 13 + [i32, _vp], _int),
        "lg_lstm_actor_create": ([_P(i32), i32, _P(_vp)], _int),
        "lg_lstm_actor_load_device": ([_vp, _P(_vp), _P(_vp), _vp, _vp], _int),
        "lg_lstm_actor_destroy": ([_vp], _int),
        "lg_lstm_actor_act": ([_vp, _vp, _vp, _vp, i32, u64, i64, _vp, i32, _vp], _int),
    }, None, ()),
}
(EXPORTED_SYMBOLS, GAME_SYMBOLS, DEC_GAME_SYMBOLS, PURSUER_SYMBOLS, OUTCOME_SYMBOLS, DEC_OUTCOME_SYMBOLS, DEC_POOL_SYMBOLS, DEC_MEMBER_OUTCOME_SYMBOLS,
 RECURRENT_SYMBOLS) = (list(functions) for functions, _, _ in ABI.values())
ALL_SYMBOLS = [symbol for functions, _, _ in ABI.values() for symbol in functions]
# what the CPU oracle exports of legged_hip.h under its own prefix: the simulator, sized by the first four structs
ORACLE_SYMBOLS = ("lg_create", "lg_destroy", "lg_bind", "lg_step", "lg_reset_idx", "lg_actuator_forward", "lg_physics_substep",
                  "lg_compute_observations_only", "lg_set_params", "lg_set_obs_buffer", "lg_last_error", "lg_abi_version", "lg_sizeof")


def bind_header(lib, header: str, prefix: str = "lg_"):
    """Attach argtypes/restype for the entry points of ``header`` and check its struct layouts.  Another ``prefix`` than ``lg_`` is the
    CPU oracle's build of legged_hip.h."""
    functions, sizeof, structs = ABI[header]
    if prefix != "lg_":
        functions, structs = {symbol: functions[symbol] for symbol in ORACLE_SYMBOLS}, structs[:4]
    for symbol, (argtypes, restype) in functions.items():
        fn = getattr(lib, prefix + symbol[3:])
        fn.argtypes, fn.restype = argtypes, restype
    for which, st in enumerate(structs):
        size = getattr(lib, prefix + sizeof[3:])(which)
        if size != C.sizeof(st):
            raise RuntimeError(f"struct layout mismatch for {st.__name__}: C {size} vs ctypes {C.sizeof(st)}")
    return lib


def bind_prototypes(lib, prefix: str):
    """``bind_header`` for legged_hip.h, under the name the oracle's loader calls."""
    return bind_header(lib, "legged_hip.h", prefix)


def bind_all(lib):
    for header in ABI:
        bind_header(lib, header)
    return lib


def _check_abi_version(lib):
    if lib.lg_abi_version() != LG_ABI_VERSION:
        raise RuntimeError("liblegged_hip.so ABI version mismatch; rebuild")


LIBRARIES["main"] = Library("liblegged_hip.so", "LG_HIP_LIB", {symbol: sig for functions, _, _ in ABI.values() for symbol, sig in functions.items()},
                            "_lib", what="the HIP extension", bind_hook=bind_all, check=_check_abi_version)


# ---------------------------------------------------------------------------------------------------------------- legged_lstm_sequence.h
# A library of its own (csrc/liblegged_lstm_seq.so, built by a second hipcc command): outside ABI / ALL_SYMBOLS / bind_all, which
# describe liblegged_hip.so.
LG_LSTM_SEQ_MAX_IN, LG_LSTM_SEQ_MAX_HIDDEN, LG_LSTM_SEQ_BLOCK_ROWS = 256, 256, 32
LSTM_SEQ_ABI = {
    "lg_lstm_seq_create": ([i32, i32, i32, _P(_vp)], _int),
    "lg_lstm_seq_load_device": ([_vp, _vp, _vp, _vp, _vp, _vp], _int),
    "lg_lstm_seq_destroy": ([_vp], _int),
    "lg_lstm_seq_workspace_floats": ([i32, i32, i32], C.c_size_t),
    "lg_lstm_seq_forward": ([_vp, _vp, i64, _vp, _vp, _vp, _vp, i32, i32, _vp], _int),
    "lg_lstm_seq_backward": ([_vp, _vp, _vp, _vp, _vp, i32, i32, _vp], _int),
    "lg_lstm_seq_last_error": ([], C.c_char_p),
}
LSTM_SEQ_SYMBOLS = list(LSTM_SEQ_ABI)
LIBRARIES["lstm_seq"] = Library("liblegged_lstm_seq.so", "LG_LSTM_SEQ_LIB", LSTM_SEQ_ABI, "_lstm_seq_lib", what="the LSTM sequence kernels")
lstm_seq_library_path, bind_lstm_seq, load_lstm_seq_library = _library_names("lstm_seq")


def lstm_seq_supported(num_in: int, hidden: int) -> bool:
    """The shapes ``lg_lstm_seq_create`` takes (the rollout cell's)."""
    return 1 <= num_in <= LG_LSTM_SEQ_MAX_IN and 32 <= hidden <= LG_LSTM_SEQ_MAX_HIDDEN and hidden % 32 == 0


# ---------------------------------------------------------------------------------------------------------------- legged_game_recurrent.h
# The recurrent actor launch of the game tasks, a library of its own as well (csrc/liblegged_game_recurrent.so, a third hipcc command):
# outside ABI / ALL_SYMBOLS / bind_all.  It reads the lg_policy / lg_lstm_actor handles liblegged_hip.so created.
GAME_RECURRENT_ABI = {
    "lg_game_lstm_act": ([_vp, _vp, _P(lg_game_params), _P(lg_game_buffers), _vp, _vp, _vp, _vp, _vp, u64, i64, _vp, i32, _vp, _vp, _vp, _vp, _vp], _int),
    "lg_game_recurrent_last_error": ([], C.c_char_p),
    "lg_game_recurrent_sizeof": _SIZEOF,
}
GAME_RECURRENT_SYMBOLS = list(GAME_RECURRENT_ABI)
GAME_RECURRENT_STRUCTS = (lg_game_params, lg_game_buffers)          # what lg_game_recurrent_sizeof sizes by index (2, 3: the two handles, opaque here)
LIBRARIES["game_recurrent"] = Library("liblegged_game_recurrent.so", "LG_GAME_RECURRENT_LIB", GAME_RECURRENT_ABI, "_game_recurrent_lib", sizeof=("lg_game_recurrent_sizeof", dict(enumerate(GAME_RECURRENT_STRUCTS))), what="the recurrent actor launch of the game tasks")
game_recurrent_library_path, bind_game_recurrent, load_game_recurrent_library = _library_names("game_recurrent")


def game_lstm_act(hl_actor, ll_policy, params: lg_game_params, buffers: lg_game_buffers, h: int, hl_obs: Optional[int], ll_obs: int, ll_actions: int,
                  mean: int, seed: int, step: int, step_counter: Optional[int], deterministic: bool, sample: Optional[int] = None,
                  sigma: Optional[int] = None, log_prob: Optional[int] = None, obs_copy: Optional[int] = None, stream: int = 0) -> int:
    """``lg_game_lstm_act``: ``lg_game_act`` for a recurrent high-level actor (an ``lg_lstm_actor`` handle on the actor memory's ``h``).
    Returns 0, or -4 when the actor pair has no shared kernel (the caller then issues the separate launches); raises on any other error."""
    lib = load_game_recurrent_library()
    rc = lib.lg_game_lstm_act(hl_actor, ll_policy, C.byref(params), C.byref(buffers), h, hl_obs, ll_obs, ll_actions, mean, int(seed), int(step),
                              step_counter, int(bool(deterministic)), sample, sigma, log_prob, obs_copy, stream)
    if rc not in (0, -4):
        raise RuntimeError(f"lg_game_lstm_act failed ({rc}): {lib.lg_game_recurrent_last_error().decode()}")
    return rc


# ---------------------------------------------------------------------------------------------------------------- legged_dec_game_recurrent.h
# The recurrent policy stage of dec_high_level_game, a fourth library (csrc/liblegged_dec_game_recurrent.so): outside ABI / ALL_SYMBOLS /
# bind_all.  It reads the lg_lstm / lg_lstm_actor / lg_policy handles liblegged_hip.so created.
class lg_dec_lstm_role(C.Structure):
    """include/legged_dec_game_recurrent.h: lg_dec_lstm_role (one memory of the cell launch: handle or None, device addresses)."""
    _fields_ = [("l", C.c_void_p), ("x", C.c_void_p), ("h_in", C.c_void_p), ("c_in", C.c_void_p), ("h_out", C.c_void_p), ("c_out", C.c_void_p)]


DEC_GAME_RECURRENT_ABI = {
    "lg_dec_lstm_step": ([_P(lg_dec_lstm_role), _vp, i32, _vp], _int),
    "lg_dec_game_lstm_act": ([_vp, _vp, _vp, _P(lg_dec_game_params), _P(lg_dec_game_buffers), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, u64, u64, i64, _vp,
                              i32, i32, _P(lg_dec_act_outputs), _P(lg_dec_act_outputs), _vp], _int),
    "lg_dec_game_recurrent_last_error": ([], C.c_char_p),
    "lg_dec_game_recurrent_sizeof": _SIZEOF,
}
DEC_GAME_RECURRENT_SYMBOLS = list(DEC_GAME_RECURRENT_ABI)
# what lg_dec_game_recurrent_sizeof sizes by index (3, 4, 5: the three handles, opaque here)
DEC_GAME_RECURRENT_STRUCTS = {0: lg_dec_game_params, 1: lg_dec_game_buffers, 2: lg_dec_act_outputs, 6: lg_dec_lstm_role}
DEC_LSTM_ROLES = ("pred_actor", "pred_critic", "prey_actor", "prey_critic")      # the order of lg_dec_lstm_step's roles
LIBRARIES["dec_game_recurrent"] = Library("liblegged_dec_game_recurrent.so", "LG_DEC_GAME_RECURRENT_LIB", DEC_GAME_RECURRENT_ABI, "_dec_game_recurrent_lib", sizeof=("lg_dec_game_recurrent_sizeof", DEC_GAME_RECURRENT_STRUCTS), what="the recurrent policy stage of dec_high_level_game")
dec_game_recurrent_library_path, bind_dec_game_recurrent, load_dec_game_recurrent_library = _library_names("dec_game_recurrent")


def dec_lstm_roles(roles, entry: str = "lg_dec_lstm_step") -> "C.Array":
    """``lg_dec_lstm_role[4]`` from four entries in the order of ``DEC_LSTM_ROLES``: None (absent), or
    ``(handle, x, h_in, c_in, h_out, c_out)`` with device addresses.  ``entry``: the entry point a wrong count is reported for."""
    if len(roles) != 4:
        raise ValueError(f"{entry} takes four roles (None = absent)")
    arr = (lg_dec_lstm_role * 4)()
    for slot, role in zip(arr, roles):
        if role is not None:
            slot.l, slot.x, slot.h_in, slot.c_in, slot.h_out, slot.c_out = (getattr(v, "value", v) for v in role)
    return arr


def dec_lstm_step(roles, reset: Optional[int], num_envs: int, stream: int = 0) -> None:
    """``lg_dec_lstm_step``: up to four memories advanced in one launch.  ``roles``: what ``dec_lstm_roles`` takes, or its result (kept by
    a caller that replays the same launch)."""
    lib = load_dec_game_recurrent_library()
    arr = roles if isinstance(roles, C.Array) else dec_lstm_roles(roles)
    rc = lib.lg_dec_lstm_step(arr, reset, int(num_envs), stream)
    if rc != 0:
        raise RuntimeError(f"lg_dec_lstm_step failed ({rc}): {lib.lg_dec_game_recurrent_last_error().decode()}")


def dec_game_lstm_act(pred_actor, prey_actor, ll_policy, params: lg_dec_game_params, buffers: lg_dec_game_buffers, h_pred: int, h_prey: int,
                      pred_obs: Optional[int], prey_obs: Optional[int], ll_obs: int, ll_actions: int, mean_pred: int, mean_prey: int, seed_pred: int,
                      seed_prey: int, step: int, step_counter: Optional[int], deterministic_pred: bool, deterministic_prey: bool,
                      out_pred: Optional[lg_dec_act_outputs] = None, out_prey: Optional[lg_dec_act_outputs] = None, stream: int = 0) -> int:
    """``lg_dec_game_lstm_act``: ``lg_dec_game_act`` for recurrent agents (``lg_lstm_actor`` handles on the actor memories' ``h``).
    Returns 0, or -4 when the actors have no shared kernel (the caller then issues the separate launches); raises on any other error."""
    lib = load_dec_game_recurrent_library()
    rc = lib.lg_dec_game_lstm_act(pred_actor, prey_actor, ll_policy, C.byref(params), C.byref(buffers), h_pred, h_prey, pred_obs, prey_obs, ll_obs, ll_actions,
                                  mean_pred, mean_prey, int(seed_pred), int(seed_prey), int(step), step_counter, int(bool(deterministic_pred)),
                                  int(bool(deterministic_prey)), C.byref(out_pred) if out_pred is not None else None,
                                  C.byref(out_prey) if out_prey is not None else None, stream)
    if rc not in (0, -4):
        raise RuntimeError(f"lg_dec_game_lstm_act failed ({rc}): {lib.lg_dec_game_recurrent_last_error().decode()}")
    return rc


# ---------------------------------------------------------------------------------------------------------------- legged_dec_pool_recurrent.h
# The recurrent policy stage of dec_high_level_game with an opponent pool, a fifth library (csrc/liblegged_dec_pool_recurrent.so): outside
# ABI / ALL_SYMBOLS / bind_all.  It reads the lg_lstm / lg_lstm_actor / lg_policy handles liblegged_hip.so created.
class lg_dec_rpool_info(C.Structure):
    """include/legged_dec_pool_recurrent.h: lg_dec_rpool_info (what ``lg_dec_rpool_query`` reports)."""
    _fields_ = [("count", i32), ("role", i32), ("device", i32), ("num_in", i32), ("hidden", i32), ("ksteps", i32), ("dims", i32 * 5), ("max_width", i32),
                ("table", C.c_void_p)]


DEC_POOL_RECURRENT_ABI = {
    "lg_dec_rpool_create": ([_P(_vp), _P(_vp), i32, i32, i32, _P(_vp)], _int),
    "lg_dec_rpool_destroy": ([_vp], _int),
    "lg_dec_rpool_query": ([_vp, _P(lg_dec_rpool_info)], _int),
    "lg_dec_pool_lstm_step": ([_P(lg_dec_lstm_role), _vp, _vp, _vp, _vp, _vp, i32, _vp], _int),
    "lg_dec_pool_lstm_act": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(lg_dec_game_params), _P(lg_dec_game_buffers), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                              u64, u64, i64, _vp, i32, i32, _P(lg_dec_act_outputs), _P(lg_dec_act_outputs), _vp], _int),
    "lg_dec_pool_recurrent_last_error": ([], C.c_char_p),
    "lg_dec_pool_recurrent_sizeof": _SIZEOF,
}
DEC_POOL_RECURRENT_SYMBOLS = list(DEC_POOL_RECURRENT_ABI)
# what lg_dec_pool_recurrent_sizeof sizes by index (3, 4, 5: the three handles, opaque here)
DEC_POOL_RECURRENT_STRUCTS = {0: lg_dec_game_params, 1: lg_dec_game_buffers, 2: lg_dec_act_outputs, 6: lg_dec_lstm_role, 7: lg_dec_rpool_info}
LIBRARIES["dec_pool_recurrent"] = Library("liblegged_dec_pool_recurrent.so", "LG_DEC_POOL_RECURRENT_LIB", DEC_POOL_RECURRENT_ABI, "_dec_pool_recurrent_lib", sizeof=("lg_dec_pool_recurrent_sizeof", DEC_POOL_RECURRENT_STRUCTS), what="the pooled recurrent policy stage of dec_high_level_game")
dec_pool_recurrent_library_path, bind_dec_pool_recurrent, load_dec_pool_recurrent_library = _library_names("dec_pool_recurrent")


def _dec_pool_recurrent_call(name, *args, ok=(0,)):
    lib = load_dec_pool_recurrent_library()
    rc = getattr(lib, name)(*args)
    if rc not in ok:
        raise RuntimeError(f"{name} failed ({rc}): {lib.lg_dec_pool_recurrent_last_error().decode()}")
    return rc


def dec_rpool_create(lstm_handles, actor_handles, role: str, device: int = 0) -> C.c_void_p:
    """``lg_dec_rpool_create`` over the members' ``lg_lstm`` (ACTOR memory) and ``lg_lstm_actor`` handles; ``role`` is "prey" or "pred".  The
    handles must outlive the pool and must not be re-created (``load_device`` / ``sync_device`` repack in place, which the pool follows)."""
    if len(lstm_handles) != len(actor_handles):
        raise ValueError("one lg_lstm and one lg_lstm_actor handle per member")
    arrays = [(C.c_void_p * len(hs))(*[getattr(h, "value", h) for h in hs]) for hs in (lstm_handles, actor_handles)]
    out = C.c_void_p()
    _dec_pool_recurrent_call("lg_dec_rpool_create", arrays[0], arrays[1], len(lstm_handles), DEC_POOL_ROLES[role], int(device), C.byref(out))
    return out


def dec_rpool_destroy(pool):
    if pool:
        load_dec_pool_recurrent_library().lg_dec_rpool_destroy(pool)


def dec_rpool_query(pool) -> lg_dec_rpool_info:
    info = lg_dec_rpool_info()
    _dec_pool_recurrent_call("lg_dec_rpool_query", pool, C.byref(info))
    return info


def dec_pool_lstm_step(roles, pool_pred, block_slot_pred: Optional[int], pool_prey, block_slot_prey: Optional[int], reset: Optional[int], num_envs: int,
                       stream: int = 0) -> None:
    """``lg_dec_pool_lstm_step``: ``lg_dec_lstm_step`` with the weights of a pooled ACTOR memory chosen per 32-env block.  ``roles`` as for
    ``dec_lstm_step`` (a pooled role's handle may be None: give its five buffers); ``pool_*``: an ``lg_dec_rpool`` handle or None,
    ``block_slot_*``: the device address of its int32 slot table."""
    arr = roles if isinstance(roles, C.Array) else dec_lstm_roles(roles, "lg_dec_pool_lstm_step")
    _dec_pool_recurrent_call("lg_dec_pool_lstm_step", arr, pool_pred, block_slot_pred, pool_prey, block_slot_prey, reset, int(num_envs), stream)


def dec_pool_lstm_act(pred_actor, prey_actor, ll_policy, pool_pred, block_slot_pred: Optional[int], pool_prey, block_slot_prey: Optional[int],
                      params: lg_dec_game_params, buffers: lg_dec_game_buffers, h_pred: int, h_prey: int, pred_obs: Optional[int], prey_obs: Optional[int],
                      ll_obs: int, ll_actions: int, mean_pred: int, mean_prey: int, seed_pred: int, seed_prey: int, step: int, step_counter: Optional[int],
                      deterministic_pred: bool, deterministic_prey: bool, out_pred: Optional[lg_dec_act_outputs] = None,
                      out_prey: Optional[lg_dec_act_outputs] = None, stream: int = 0) -> int:
    """``lg_dec_pool_lstm_act``: ``lg_dec_game_lstm_act`` with the actor MLP of a pooled role chosen per 32-env block.  Returns 0, or -4 when
    the actors have no shared kernel (the caller then issues the separate launches); raises on any other error."""
    return _dec_pool_recurrent_call("lg_dec_pool_lstm_act", pred_actor, prey_actor, ll_policy, pool_pred, block_slot_pred, pool_prey, block_slot_prey,
                                    C.byref(params), C.byref(buffers), h_pred, h_prey, pred_obs, prey_obs, ll_obs, ll_actions, mean_pred, mean_prey,
                                    int(seed_pred), int(seed_prey), int(step), step_counter, int(bool(deterministic_pred)), int(bool(deterministic_prey)),
                                    C.byref(out_pred) if out_pred is not None else None, C.byref(out_prey) if out_prey is not None else None, stream,
                                    ok=(0, -4))


# ---------------------------------------------------------------------------------------------------------------- legged_dec_game_privileged.h
# The privileged (critic-only) observations of dec_high_level_game, a sixth library (csrc/liblegged_dec_game_privileged.so): outside ABI /
# ALL_SYMBOLS / bind_all.  It reads lg_dec_game_params / lg_dec_game_buffers and no handle of the other libraries.
LG_DEC_NUM_PRIV_PREY, LG_DEC_NUM_PRIV_PRED = 22, 10
DEC_GAME_PRIVILEGED_ABI = {
    "lg_dec_game_privileged_obs": ([_P(lg_dec_game_params), _P(lg_dec_game_buffers), _vp, _vp, _vp], _int),
    "lg_dec_game_privileged_last_error": ([], C.c_char_p),
    "lg_dec_game_privileged_sizeof": _SIZEOF,
}
DEC_GAME_PRIVILEGED_SYMBOLS = list(DEC_GAME_PRIVILEGED_ABI)
DEC_GAME_PRIVILEGED_STRUCTS = {0: lg_dec_game_params, 1: lg_dec_game_buffers}      # what lg_dec_game_privileged_sizeof sizes by index
LIBRARIES["dec_game_privileged"] = Library("liblegged_dec_game_privileged.so", "LG_DEC_GAME_PRIVILEGED_LIB", DEC_GAME_PRIVILEGED_ABI, "_dec_game_privileged_lib", sizeof=("lg_dec_game_privileged_sizeof", DEC_GAME_PRIVILEGED_STRUCTS), what="the privileged observations of dec_high_level_game")
dec_game_privileged_library_path, bind_dec_game_privileged, load_dec_game_privileged_library = _library_names("dec_game_privileged")


def dec_game_privileged_obs(params: lg_dec_game_params, buffers: lg_dec_game_buffers, priv_pred: Optional[int], priv_prey: Optional[int],
                            stream: int = 0) -> None:
    """``lg_dec_game_privileged_obs``: the critic-only rows of either agent ([N,10] / [N,22] device addresses, None = not written) from the
    state the post launch left."""
    lib = load_dec_game_privileged_library()
    rc = lib.lg_dec_game_privileged_obs(C.byref(params), C.byref(buffers), priv_pred, priv_prey, stream)
    if rc != 0:
        raise RuntimeError(f"lg_dec_game_privileged_obs failed ({rc}): {lib.lg_dec_game_privileged_last_error().decode()}")


# ---------------------------------------------------------------------------------------------------------------- legged_recurrent_wide.h
# The LSTM cell and actor MLP of memories with up to 512 units, a seventh library (csrc/liblegged_lstm_wide.so): outside ABI / ALL_SYMBOLS /
# bind_all.  Its handles are its own; the signatures are those of the lg_lstm_* entries of legged_recurrent.h.
LG_LSTM_WIDE_MAX_IN, LG_LSTM_WIDE_MAX_HIDDEN, LG_LSTM_WIDE_GROUP_UNITS, LG_LSTM_WIDE_BLOCK_ENVS = 256, 512, 256, 32
LSTM_WIDE_ABI = {
    "lg_lstm_wide_create": ([i32, i32, _vp, _vp, _vp, _vp, i32, _P(_vp)], _int),
    "lg_lstm_wide_load_device": ([_vp, _vp, _vp, _vp, _vp, _vp], _int),
    "lg_lstm_wide_destroy": ([_vp], _int),
    "lg_lstm_wide_step": ([_vp] * 13 + [i32, _vp], _int),
    "lg_lstm_wide_actor_create": ([_P(i32), i32, _P(_vp)], _int),
    "lg_lstm_wide_actor_load_device": ([_vp, _P(_vp), _P(_vp), _vp, _vp], _int),
    "lg_lstm_wide_actor_destroy": ([_vp], _int),
    "lg_lstm_wide_actor_act": ([_vp, _vp, _vp, _vp, i32, u64, i64, _vp, i32, _vp], _int),
    "lg_lstm_wide_last_error": ([], C.c_char_p),
}
LSTM_WIDE_SYMBOLS = list(LSTM_WIDE_ABI)
LIBRARIES["lstm_wide"] = Library("liblegged_lstm_wide.so", "LG_LSTM_WIDE_LIB", LSTM_WIDE_ABI, "_lstm_wide_lib", what="the wide LSTM cell and actor")
lstm_wide_library_path, bind_lstm_wide, load_lstm_wide_library = _library_names("lstm_wide")


def lstm_wide_supported(num_in: int, hidden: int) -> bool:
    """The shapes ``lg_lstm_wide_create`` takes."""
    return 1 <= num_in <= LG_LSTM_WIDE_MAX_IN and 32 <= hidden <= LG_LSTM_WIDE_MAX_HIDDEN and hidden % 32 == 0


# ----------------------------------------------------------------------------------------------------------------- legged_recurrent_gru.h
# The GRU cell of a recurrent policy, an eighth library (csrc/liblegged_gru.so): outside ABI / ALL_SYMBOLS / bind_all.  Its handles are its
# own; the actor MLP behind a GRU memory is the main library's lg_lstm_actor.
LG_GRU_MAX_IN, LG_GRU_MAX_HIDDEN, LG_GRU_BLOCK_ENVS = 256, 256, 32
GRU_ABI = {
    "lg_gru_create": ([i32, i32, _vp, _vp, _vp, _vp, i32, _P(_vp)], _int),
    "lg_gru_load_device": ([_vp, _vp, _vp, _vp, _vp, _vp], _int),
    "lg_gru_destroy": ([_vp], _int),
    "lg_gru_step": ([_vp] * 9 + [i32, _vp], _int),
    "lg_gru_last_error": ([], C.c_char_p),
}
GRU_SYMBOLS = list(GRU_ABI)
LIBRARIES["gru"] = Library("liblegged_gru.so", "LG_GRU_LIB", GRU_ABI, "_gru_lib", what="the GRU cell")
gru_library_path, bind_gru, load_gru_library = _library_names("gru")


def gru_supported(num_in: int, hidden: int) -> bool:
    """The shapes ``lg_gru_create`` takes."""
    return 1 <= num_in <= LG_GRU_MAX_IN and 32 <= hidden <= LG_GRU_MAX_HIDDEN and hidden % 32 == 0


# ----------------------------------------------------------------------------------------------------------------- legged_dec_game_gru.h
# The shared cell launch of GRU policies on dec_high_level_game, a ninth library (csrc/liblegged_dec_game_gru.so): outside ABI / ALL_SYMBOLS
# / bind_all.  It reads the lg_gru handles liblegged_gru.so created.
class lg_gru_handle(C.Structure):
    """csrc/lg_gru.h: struct lg_gru (opaque to callers; here for the size check of ``bind_dec_game_gru``)."""
    _fields_ = [("num_in", i32), ("hidden", i32), ("ksteps", i32), ("device", i32), ("d_wp", C.c_void_p), ("d_bp", C.c_void_p)]


class lg_dec_gru_role(C.Structure):
    """include/legged_dec_game_gru.h: lg_dec_gru_role (one memory of the cell launch: handle or None, device addresses)."""
    _fields_ = [("l", C.c_void_p), ("x", C.c_void_p), ("h_in", C.c_void_p), ("h_out", C.c_void_p)]


DEC_GAME_GRU_ABI = {
    "lg_dec_gru_step": ([_P(lg_dec_gru_role), _vp, i32, _vp], _int),
    "lg_dec_game_gru_last_error": ([], C.c_char_p),
    "lg_dec_game_gru_sizeof": _SIZEOF,
}
DEC_GAME_GRU_SYMBOLS = list(DEC_GAME_GRU_ABI)
DEC_GAME_GRU_STRUCTS = {0: lg_gru_handle, 1: lg_dec_gru_role}      # what lg_dec_game_gru_sizeof sizes by index
LIBRARIES["dec_game_gru"] = Library("liblegged_dec_game_gru.so", "LG_DEC_GAME_GRU_LIB", DEC_GAME_GRU_ABI, "_dec_game_gru_lib", sizeof=("lg_dec_game_gru_sizeof", DEC_GAME_GRU_STRUCTS), what="the shared GRU cell launch of dec_high_level_game")
dec_game_gru_library_path, bind_dec_game_gru, load_dec_game_gru_library = _library_names("dec_game_gru")


def dec_gru_roles(roles) -> "C.Array":
    """``lg_dec_gru_role[4]`` from four entries in the order of ``DEC_LSTM_ROLES``: None (absent), or ``(handle, x, h_in, h_out)`` with
    device addresses."""
    if len(roles) != 4:
        raise ValueError("lg_dec_gru_step takes four roles (None = absent)")
    arr = (lg_dec_gru_role * 4)()
    for slot, role in zip(arr, roles):
        if role is not None:
            slot.l, slot.x, slot.h_in, slot.h_out = (getattr(v, "value", v) for v in role)
    return arr


def dec_gru_step(roles, reset: Optional[int], num_envs: int, stream: int = 0) -> None:
    """``lg_dec_gru_step``: up to four GRU memories advanced in one launch.  ``roles``: what ``dec_gru_roles`` takes, or its result (kept by
    a caller that replays the same launch)."""
    lib = load_dec_game_gru_library()
    arr = roles if isinstance(roles, C.Array) else dec_gru_roles(roles)
    rc = lib.lg_dec_gru_step(arr, reset, int(num_envs), stream)
    if rc != 0:
        raise RuntimeError(f"lg_dec_gru_step failed ({rc}): {lib.lg_dec_game_gru_last_error().decode()}")


class Sim:
    """Owner of one ``lg_sim`` handle (one per GPU).  ``lib``/``prefix`` are
    parameters only so the tests can drive the CPU oracle through the same class."""

    def __init__(self, params: lg_params, model: lg_robot_model, actuator_weights: Optional[np.ndarray],
                 device_id: int = 0, lib=None, prefix: str = "lg_"):
        self.lib = lib if lib is not None else load_library()
        self.prefix = prefix
        self.params, self.model = params, model
        self._w = None
        wptr = None
        if actuator_weights is not None:
            self._w = np.ascontiguousarray(actuator_weights, dtype=np.float32)
            if self._w.size != LG_ACTUATOR_FLOATS:
                raise ValueError("actuator weight blob must hold 972 floats")
            wptr = self._w.ctypes.data_as(_PF)
        self.handle = C.c_void_p()
        self._check(self._fn("create")(C.byref(params), C.byref(model), wptr, int(device_id), C.byref(self.handle)))
        self.buffers = lg_buffers()

    def _fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"{self.prefix}* call failed ({rc}): {self._fn('last_error')().decode()}")

    def bind(self, pointers: Dict[str, int]):
        self.buffers = _buffers(lg_buffers, pointers)
        self._check(self._fn("bind")(self.handle, C.byref(self.buffers)))

    def step(self, actions_ptr: int, common_step_counter: int, stream: int = 0):
        self._check(self._fn("step")(self.handle, actions_ptr, int(common_step_counter), stream))

    def step_policy(self, policy_handle, obs_ptr: int, actions_ptr: int, mean_ptr, seed: int, deterministic: bool,
                    common_step_counter: int, stream: int = 0):
        self._check(self.lib.lg_step_policy(self.handle, policy_handle, obs_ptr, actions_ptr, mean_ptr, int(seed), int(bool(deterministic)),
                                            int(common_step_counter), stream))

    def rollout_policy(self, policy_handle, steps: int, obs_ptr: int, actions_ptr: int, mean_ptr, rew_ptr: int, dones_ptr: int, time_outs_ptr: int,
                       seed: int, deterministic: bool, common_step_counter: int, stream: int = 0, obs0_ptr=None):
        pointers = {"obs": obs_ptr, "obs0": obs0_ptr, "actions": actions_ptr, "mean": mean_ptr, "rew": rew_ptr, "dones": dones_ptr, "time_outs": time_outs_ptr}
        r = _buffers(lg_rollout_buffers, pointers, pointers)
        r.steps = int(steps)
        self._check(self.lib.lg_rollout_policy(self.handle, policy_handle, C.byref(r), int(seed), int(bool(deterministic)), int(common_step_counter), stream))

    def set_deferred_extras(self, on: bool):
        self._check(self.lib.lg_set_deferred_extras(self.handle, int(bool(on))))

    def extras_flush(self, common_step_counter: int, stream: int = 0):
        self._check(self.lib.lg_extras_flush(self.handle, int(common_step_counter), stream))

    def reset_idx(self, ids_ptr: int, count: int, common_step_counter: int, stream: int = 0):
        self._check(self._fn("reset_idx")(self.handle, ids_ptr, int(count), int(common_step_counter), stream))

    def actuator_forward(self, pos_err, vel, torques, hidden, cell, rows, stream=0):
        self._check(self._fn("actuator_forward")(self.handle, pos_err, vel, torques, hidden, cell, int(rows), stream))

    def physics_substep(self, torques_ptr, write_contacts=1, stream=0):
        self._check(self._fn("physics_substep")(self.handle, torques_ptr, int(write_contacts), stream))

    def compute_observations_only(self, common_step_counter, stream=0):
        self._check(self._fn("compute_observations_only")(self.handle, int(common_step_counter), stream))

    def set_obs_buffer(self, ptr: int):
        self._check(self._fn("set_obs_buffer")(self.handle, ptr))

    def set_params(self, params: lg_params):
        self.params = params
        self._check(self._fn("set_params")(self.handle, C.byref(params)))

    def resample_reset_commands(self, common_step_counter: int, stream: int = 0):
        self._check(self.lib.lg_resample_reset_commands(self.handle, int(common_step_counter), stream))

    def device_status(self, synchronize: bool = True) -> int:
        """``lg_device_status``: the sticky status word of the handle (0 = clean); see include/legged_hip.h."""
        return int(self.lib.lg_device_status(self.handle, int(bool(synchronize))))

    def clear_device_status(self):
        self._check(self.lib.lg_clear_device_status(self.handle))

    def debug_handover(self, skip: int, spin_limit: int = 0):
        self._check(self.lib.lg_debug_handover(self.handle, int(skip), int(spin_limit)))

    def close(self):
        if self.handle:
            self._fn("destroy")(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
