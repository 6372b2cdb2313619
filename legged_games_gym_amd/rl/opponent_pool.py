"""``OpponentPool``: the opponent of a learning agent of ``dec_high_level_game`` as a mixture -- the live opponent in part of the envs, frozen
earlier versions of it in the rest -- in ONE actor launch (``lg_dec_pool_act``, include/legged_dec_game_pool.h).

A role's workgroup of the shared actor launch serves 32 envs, so the unit of the mixture is the 32-env block: a device table names, for every
block, the pool member whose weights, biases and std the block's workgroup streams.  Member 0 is the live opponent's ``FusedActor`` (its
weights keep following ``sync_device()``); members 1 .. ``capacity`` are ``FusedActor`` s over private ``ActorCritic`` copies, created once, so
the C-side table of operand addresses never changes: ``push`` loads a snapshot into the next ring slot IN PLACE, and ``assign`` rewrites the
slot table IN PLACE -- both are visible underneath a captured graph at its next replay.

``DecHighLevelGame.step_policy`` / ``make_graphed_policy_step`` and ``AgentView.step_policy`` accept a pool wherever they accept a
``FusedActor`` opponent; the pool's ``live`` actor supplies the noise seed, the step source and the output buffers.

Outcomes per member (include/legged_dec_game_member_outcome.h): the pool owns the device counts ``member_totals``
``[16, 6]`` that ``lg_dec_member_outcome_post`` keeps once ``DecHighLevelGame.enable_member_outcomes(pool)`` has bound the pool.  They feed the
prioritised deal: ``learner_win_rate`` -> ``pfsp_weights`` -> ``apportion`` -> ``assign_blocks_weighted`` (``assign(weights=...)``).

``RecurrentOpponentPool`` is the same pool for ``ActorCriticRecurrent`` policies (``lg_dec_pool_lstm_step`` / ``lg_dec_pool_lstm_act``,
include/legged_dec_pool_recurrent.h): both share ``PoolBase``; ``stale_blocks`` is the rule by which a re-deal zeroes the memory of a block whose member
changed or was overwritten."""
from fractions import Fraction

import torch

from .. import capi

BLOCK = capi.LG_DEC_POOL_BLOCK_ENVS


def assign_blocks(num_blocks, filled, latest_share, generator):
    """The slot of every 32-env block, an int32 CPU tensor ``[num_blocks]`` with values in ``0 .. filled``: 0 is the live member, ``s >= 1``
    snapshot ``s``.  ``latest_share == 0`` gives no live block, otherwise ``max(1, round(latest_share * num_blocks))`` blocks are live; which
    ones is a permutation drawn from ``generator``, and the remaining blocks are dealt round-robin over the ``filled`` snapshots in the
    permuted order, so the snapshots' counts differ by at most one.  With ``filled == 0`` every block is live.  By block and at random, not by
    env range: terrain types are contiguous in env index, and a contiguous split would confound opponent with terrain."""
    if num_blocks < 1 or filled < 0 or not 0.0 <= latest_share <= 1.0:
        raise ValueError(f"assign_blocks: num_blocks >= 1, filled >= 0 and 0 <= latest_share <= 1, got {(num_blocks, filled, latest_share)}")
    slots = torch.zeros(num_blocks, dtype=torch.int32)
    if filled == 0:
        return slots
    perm = torch.randperm(num_blocks, generator=generator)
    live = 0 if latest_share == 0 else min(num_blocks, max(1, round(latest_share * num_blocks)))
    rest = perm[live:]
    slots[rest] = 1 + (torch.arange(len(rest), dtype=torch.int32) % filled)
    return slots


def learner_win_rate(totals_row, learner):
    """The share of the episodes of ``totals_row`` (a dict with ``episodes`` and ``captured``) that the ``learner`` ("pred" or "prey") won:
    ``captured / episodes`` for the predator, ``1 - captured / episodes`` for the prey.  The flags of an episode's end are not exclusive, so
    "not captured" is the prey's win here, whatever else ended the episode.  NaN without an episode."""
    if learner not in ("pred", "prey"):
        raise ValueError(f"learner must be 'pred' or 'prey', got {learner!r}")
    episodes, captured = int(totals_row["episodes"]), int(totals_row["captured"])
    if episodes == 0:
        return float("nan")
    rate = captured / episodes
    return rate if learner == "pred" else 1.0 - rate


def pfsp_weights(wins, episodes, power):
    """Prioritised fictitious self-play: the weight of a past opponent is ``(1 - (wins + 1) / (episodes + 2)) ** power``, ``wins`` the learner's
    wins in ``episodes`` episodes against it.  The Laplace term gives a member that has not been met a win rate of 0.5; ``power = 0`` gives
    all ones (the uniform deal).  Returns a list of floats."""
    if len(wins) != len(episodes):
        raise ValueError("pfsp_weights: wins and episodes must have one entry per member")
    if power < 0:
        raise ValueError(f"pfsp_weights: power must be >= 0, got {power}")
    out = []
    for w, n in zip(wins, episodes):
        if not 0 <= w <= n:
            raise ValueError(f"pfsp_weights: 0 <= wins <= episodes, got {(w, n)}")
        out.append(1.0 if power == 0 else (1.0 - (w + 1.0) / (n + 2.0)) ** float(power))
    return out


def apportion(weights, total):
    """Integer shares of ``total`` in proportion to ``weights`` by the largest-remainder method: the floors of the quotas, then one more to
    the largest remainders, ties going to the lower index.  When ``total >= len(weights)`` every member first gets 1 share and the rest is
    apportioned, so a member with a small weight keeps being measured.  All-zero weights count as equal.  Deterministic."""
    k, total = len(weights), int(total)
    if total < 0 or any(not w >= 0 for w in weights):
        raise ValueError(f"apportion: total >= 0 and weights >= 0, got {(list(weights), total)}")
    if k == 0:
        return []
    weights = [Fraction(float(w)) for w in weights]              # exact: the floors and the order of the remainders do not depend on rounding
    if sum(weights) <= 0:
        weights = [Fraction(1)] * k
    base = 1 if total >= k else 0
    rest, scale = total - base * k, sum(weights)
    quotas = [rest * w / scale for w in weights]
    shares = [q.numerator // q.denominator for q in quotas]
    order = sorted(range(k), key=lambda i: (-(quotas[i] - shares[i]), i))
    for i in order[:rest - sum(shares)]:
        shares[i] += 1
    return [base + s for s in shares]


def assign_blocks_weighted(num_blocks, filled, latest_share, weights, generator):
    """``assign_blocks`` with the non-live blocks dealt in proportion to ``weights`` (one per snapshot 1 .. ``filled``): the live blocks are
    drawn exactly as there, and the rest of the permuted order is cut into runs of the lengths ``apportion(weights, rest)``, snapshot 1
    first.  With equal weights the snapshots' counts are those of ``assign_blocks``."""
    if num_blocks < 1 or filled < 0 or not 0.0 <= latest_share <= 1.0:
        raise ValueError(f"assign_blocks_weighted: num_blocks >= 1, filled >= 0 and 0 <= latest_share <= 1, got {(num_blocks, filled, latest_share)}")
    if len(weights) != filled:
        raise ValueError(f"assign_blocks_weighted: one weight per filled snapshot ({filled}), got {len(weights)}")
    slots = torch.zeros(num_blocks, dtype=torch.int32)
    if filled == 0:
        return slots
    perm = torch.randperm(num_blocks, generator=generator)
    live = 0 if latest_share == 0 else min(num_blocks, max(1, round(latest_share * num_blocks)))
    rest = perm[live:]
    shares = apportion(weights, len(rest))
    slots[rest] = torch.repeat_interleave(1 + torch.arange(filled, dtype=torch.int32), torch.tensor(shares, dtype=torch.long))
    return slots


def stale_blocks(old_slots, new_slots, overwritten, count):
    """Which 32-env blocks of a pooled recurrent role hold an ``(h, c)`` state that must not be continued: a bool CPU tensor ``[blocks]``.
    ``old_slots`` / ``new_slots``: the slot tables before and after a deal, clamped to ``[0, count)`` as the kernels clamp them;
    ``overwritten``: the members whose weights were overwritten since the last deal (``push``).  A block is stale when its member changes,
    or when its member stays but was overwritten -- either way its state was produced under other weights than those that would continue it.
    Member 0, the live actor, is never stale by being overwritten: it changes every iteration, and its state carries on as it does without a
    pool.  Pure: no device, no pool."""
    old = torch.as_tensor(old_slots, dtype=torch.int64).cpu().clamp(0, int(count) - 1)
    new = torch.as_tensor(new_slots, dtype=torch.int64).cpu().clamp(0, int(count) - 1)
    if old.shape != new.shape:
        raise ValueError(f"stale_blocks: the slot tables differ in size, {tuple(old.shape)} and {tuple(new.shape)}")
    stale = old != new
    for m in sorted(set(int(m) for m in overwritten)):
        if not 0 <= m < int(count):
            raise ValueError(f"stale_blocks: overwritten member {m} outside the pool of {count}")
        if m != 0:
            stale |= new == m
    return stale


class PoolBase:
    """What ``OpponentPool`` and ``RecurrentOpponentPool`` share: member 0 the live actor, members 1 .. ``capacity`` private copies created
    once, the ring ``push``, the device slot table with ``assign`` / ``set_slots``, the outcome counts per member, ``state`` / ``load_state`` and
    the guarded ``handle``.  A subclass makes a member (``_make_member``), creates and destroys the C-side pool (``_create_pool``,
    ``_destroy_pool``) and may react to a push (``_overwritten``) and to a new slot table (``_slots_changed``)."""
    is_opponent_pool = True

    def __init__(self, live, make_actor_critic, capacity, role, seed=0, latest_share=0.5, num_envs=None):
        if role not in capi.DEC_POOL_ROLES:
            raise ValueError(f"role must be one of {tuple(capi.DEC_POOL_ROLES)}, got {role!r}")
        if not 1 <= int(capacity) <= capi.LG_DEC_POOL_MAX - 1:
            raise ValueError(f"capacity must be 1 .. {capi.LG_DEC_POOL_MAX - 1} (LG_DEC_POOL_MAX - 1: member 0 is the live actor), got {capacity}")
        self._pool = None
        self.live, self.role, self.capacity, self.seed, self.latest_share = live, role, int(capacity), int(seed), float(latest_share)
        self.device = live.device
        self.members = [live]
        for _ in range(self.capacity):
            ac = make_actor_critic()
            ac.load_state_dict(live.ac.state_dict())              # never assigned before its first push; a stale table still meets a sane actor
            self.members.append(self._make_member(ac))
        self.filled, self._next = 0, 0                           # snapshots written; ring position of the next push (member 1 + _next)
        self.pushed_at = [None] * self.capacity                  # per snapshot member 1 .. capacity: the evolution that pushed it (None: not told)
        # the six outcome counts per member (lg_dec_member_outcome_post): rows = members, never re-allocated (a captured graph holds the addresses)
        self.member_accum = torch.zeros(capi.LG_DEC_MEMBER_OUTCOME_ROWS, capi.LG_DEC_OUTCOME_NUM_COUNTS, dtype=torch.int64, device=self.device)
        self.member_totals = torch.zeros_like(self.member_accum)
        self._creations = [self._creation(m) for m in self.members]
        self._pool = self._create_pool()
        self._slots = self._slots_host = self._scratch = None
        self._assignments = 0
        if num_envs is not None:
            self.slot_table(num_envs)

    # ------------------------------------------------------------------ what a subclass supplies
    def _make_member(self, ac):
        raise NotImplementedError

    def _create_pool(self):
        raise NotImplementedError

    def _destroy_pool(self):
        raise NotImplementedError

    @staticmethod
    def _creation(member):
        """What changes when a member's C handle is re-created (the table of operand addresses would dangle)."""
        return getattr(member, "creations", 0)

    def _overwritten(self, index):
        """Member ``index`` has just been given other weights (``push``)."""

    def _slots_changed(self, old, new):
        """The slot table went from ``old`` to ``new`` (CPU int32 tensors)."""

    # ------------------------------------------------------------------ what the env reads
    @property
    def handle(self):
        """The C-side pool.  Its table holds the members' operand addresses as they were at construction: a member whose handle was
        re-created (``FusedActor.sync()``; ``sync_device()`` repacks in place) would leave it dangling."""
        if [self._creation(m) for m in self.members] != self._creations:     # (not the handles' values: a re-created handle may get the old address)
            raise RuntimeError("a member's lg_policy handle was re-created (FusedActor.sync()); a pool's members are updated with sync_device() only")
        return self._pool

    def slot_table(self, num_envs):
        """The device int32 table ``[ceil(num_envs / 32)]`` the launch reads (all live until ``assign`` / ``set_slots``)."""
        blocks = (int(num_envs) + BLOCK - 1) // BLOCK
        if self._slots is None:
            self._slots = torch.zeros(blocks, dtype=torch.int32, device=self.device)
            self._slots_host = torch.zeros(blocks, dtype=torch.int32)
        elif self._slots.shape[0] != blocks:
            raise ValueError(f"the pool's slot table serves {self._slots.shape[0]} blocks, not the {blocks} of {num_envs} envs")
        return self._slots

    def set_slots(self, slots):
        """Rewrite the slot table in place (same address: a captured graph reads the new table at its next replay)."""
        slots = torch.as_tensor(slots, dtype=torch.int32).cpu().contiguous()
        if self._slots is None:
            self._slots = torch.zeros(len(slots), dtype=torch.int32, device=self.device)
        if slots.shape != self._slots.shape:
            raise ValueError(f"the pool's slot table has {self._slots.shape[0]} blocks, got {tuple(slots.shape)}")
        old = self._slots_host if self._slots_host is not None else torch.zeros_like(slots)
        self._slots_host = slots.clone()
        self._slots.copy_(slots)
        self._slots_changed(old, self._slots_host)

    def assign(self, generator=None, weights=None):
        """Draw a new assignment of blocks to members and write it to the device table: ``assign_blocks``, or with ``weights`` (one per filled
        snapshot) ``assign_blocks_weighted``.  Returns the CPU table."""
        if self._slots is None:
            raise RuntimeError("the slot table has no size yet: construct the pool with num_envs or call slot_table(num_envs) first")
        if generator is None:
            generator = torch.Generator().manual_seed(self.seed + self._assignments)
        self._assignments += 1
        if weights is None:
            slots = assign_blocks(self._slots.shape[0], self.filled, self.latest_share, generator)
        else:
            slots = assign_blocks_weighted(self._slots.shape[0], self.filled, self.latest_share, list(weights), generator)
        self.set_slots(slots)
        return slots

    # ------------------------------------------------------------------ snapshots
    def push(self, state_dict, pushed_at=None):
        """Load ``state_dict`` (of the live actor's module) into the next ring slot, the oldest snapshot overwritten, and repack that
        member on the device -- in place, so it is visible underneath a captured graph.  ``pushed_at``: the evolution that pushes (recorded
        per snapshot).  The outcome counts of the overwritten row and of row 0 are zeroed, in place and stream-ordered: the live member is
        about to be trained, so both rows stand for new opponents.  Returns the member's index."""
        index = 1 + self._next
        member = self.members[index]
        member.ac.load_state_dict(state_dict)
        member.sync_device()
        self._overwritten(index)
        self.pushed_at[index - 1] = None if pushed_at is None else int(pushed_at)
        self.reset_member_totals(rows=(0, index))
        self._next = (self._next + 1) % self.capacity
        self.filled = min(self.filled + 1, self.capacity)
        return index

    # ------------------------------------------------------------------ outcomes per member
    def member_totals_host(self):
        """The running counts of members 0 .. ``filled`` as a list of dicts (``capi.DEC_OUTCOME_COUNTS`` -> int), after ONE synchronising copy."""
        rows = self.member_totals[:self.filled + 1].cpu().tolist()
        return [dict(zip(capi.DEC_OUTCOME_COUNTS, (int(v) for v in row))) for row in rows]

    def reset_member_totals(self, rows=None):
        """Zero the running counts of ``rows`` (all when None): in place and stream-ordered, no synchronisation."""
        if rows is None:
            self.member_totals.zero_()
        else:
            for r in rows:
                self.member_totals[int(r)].zero_()

    def state(self):
        """For checkpoints: the snapshots' state dicts (clones), ``filled``, the ring position, the evolution that pushed each snapshot (-1: not
        told) and the outcome counts per member."""
        return {"filled": self.filled, "next": self._next,
                "snapshots": [{k: v.detach().clone() for k, v in m.ac.state_dict().items()} for m in self.members[1:]],
                "pushed_at": [-1 if p is None else int(p) for p in self.pushed_at], "member_totals": self.member_totals.detach().cpu().clone()}

    def load_state(self, d):
        snapshots = d["snapshots"]
        if len(snapshots) != self.capacity:
            raise ValueError(f"the checkpoint's pool has {len(snapshots)} snapshot members, this pool {self.capacity}")
        for index, (member, sd) in enumerate(zip(self.members[1:], snapshots), start=1):
            member.ac.load_state_dict(sd)
            member.sync_device()
            self._overwritten(index)
        self.filled, self._next = int(d["filled"]), int(d["next"])
        if "pushed_at" in d:                                      # checkpoints without these keys load as before
            self.pushed_at = [None if int(p) < 0 else int(p) for p in d["pushed_at"]]
        if "member_totals" in d:
            self.member_totals.copy_(torch.as_tensor(d["member_totals"], dtype=torch.int64))

    def __del__(self):
        try:
            self._destroy_pool()
        except Exception:
            pass


class OpponentPool(PoolBase):
    def __init__(self, live, make_actor_critic, capacity, role, seed=0, latest_share=0.5, num_envs=None):
        """``live``: the opponent's current ``FusedActor``.  ``make_actor_critic``: zero-argument factory of an ``ActorCritic`` of the live one's
        shape on its device (one private copy per snapshot member).  ``role``: "prey" or "pred", the role the pool's members play.  ``seed``
        seeds ``assign()`` when it is called without a generator.  ``num_envs`` sizes the slot table (otherwise the first use does)."""
        super().__init__(live, make_actor_critic, capacity, role, seed=seed, latest_share=latest_share, num_envs=num_envs)

    def _make_member(self, ac):
        from .fused_actor import FusedActor
        return FusedActor(ac, self.device, seed=self.live.seed, step_counter=self.live.step_counter)

    def _create_pool(self):
        return capi.dec_pool_create([m.handle.value for m in self.members], self.role, self.device.index or 0)

    def _destroy_pool(self):
        capi.dec_pool_destroy(self._pool)

    # ------------------------------------------------------------------ separate launches (no shared kernel: wide precision 0)
    def act_separate(self, obs, deterministic):
        """What the pooled launch computes for this role without it: for every member in use one ``lg_policy_act`` on ALL envs with the live
        actor's seed and this step, rows selected by the block mask.  Returns ``(sample, mean, std)``: the first two in the live actor's
        output buffers, ``std`` [n, actions] the rows' members' std.  Counts one step of the live actor's noise stream."""
        live, n = self.live, obs.shape[0]
        lib = live.lib
        actions, mean = live.output_buffers(n)
        if self._scratch is None or self._scratch[0].shape != actions.shape:
            self._scratch = (torch.empty_like(actions), torch.empty_like(mean))
        a, mu = self._scratch
        self.slot_table(n)
        host = self._slots_host.clamp(0, self.capacity)                     # the kernel's clamp to [0, count)
        env_slot = self._slots.clamp(0, self.capacity).long().repeat_interleave(BLOCK)[:n].unsqueeze(1)
        step, ctr = live.next_step()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        std = torch.empty_like(actions)
        for k, s in enumerate(sorted(set(host.tolist()))):
            member = self.members[s]
            rc = lib.lg_policy_act(member.handle, obs.data_ptr(), a.data_ptr(), mu.data_ptr(), n, live.seed, step, ctr, int(bool(deterministic)), stream)
            if rc != 0:
                raise RuntimeError(f"lg_policy_act failed ({rc}): {lib.lg_last_error().decode()}")
            rows = env_slot == s
            member_std = member.ac.std.detach().expand(n, -1)
            if k == 0:
                actions.copy_(a); mean.copy_(mu); std.copy_(member_std)
            else:
                actions.copy_(torch.where(rows, a, actions)); mean.copy_(torch.where(rows, mu, mean)); std.copy_(torch.where(rows, member_std, std))
        return actions, mean, std


class RecurrentOpponentPool(PoolBase):
    """``OpponentPool`` for recurrent policies (include/legged_dec_pool_recurrent.h): the members are ``RecurrentFusedActor`` s over private
    ``ActorCriticRecurrent`` copies, ``live`` is the opponent's own actor, and the two pooled launches ``lg_dec_pool_lstm_step`` /
    ``lg_dec_pool_lstm_act`` take the weights of the ACTOR memory and of the actor MLP of every 32-env block from the member its slot names.

    A pooled role has ONE ``(h, c)`` ping-pong: the live actor's actor memory; the rows of block b are advanced by member ``slot[b]``.  A state
    produced under one member's weights must not be continued under another's: ``assign`` / ``set_slots`` zero, in BOTH slots, the rows of the
    blocks that ``stale_blocks`` names -- those whose member changes, and those whose member was overwritten by a ``push`` since the last
    deal.  The zeroing is in place and stream-ordered; the runner deals before it captures its graph.  Member 0, the live actor, is never
    marked: it changes every iteration, as it does without a pool."""
    recurrent = True

    def __init__(self, live, make_actor_critic, capacity, role, seed=0, latest_share=0.5, num_envs=None):
        """As ``OpponentPool``, with ``live`` a ``RecurrentFusedActor`` and ``make_actor_critic`` a factory of ``ActorCriticRecurrent`` s of its
        shape."""
        self._marked = set()                                     # members overwritten since the last deal
        super().__init__(live, make_actor_critic, capacity, role, seed=seed, latest_share=latest_share, num_envs=num_envs)
        self._said = set()

    def _make_member(self, ac):
        from .recurrent_actor import RecurrentFusedActor
        return RecurrentFusedActor(ac, self.device, seed=self.live.seed, step_counter=self.live.step_counter)

    def _create_pool(self):
        return capi.dec_rpool_create([m.lstm_a.handle for m in self.members], [m.fused.handle for m in self.members], self.role, self.device.index or 0)

    def _destroy_pool(self):
        capi.dec_rpool_destroy(self._pool)

    @property
    def _flip(self):
        """The ping-pong position of the pooled role's state: the live actor's (what ``OnPolicyRunner`` puts back after a failed capture)."""
        return self.live._flip

    @_flip.setter
    def _flip(self, value):
        self.live._flip = value

    # ------------------------------------------------------------------ a state under another member's weights
    def _overwritten(self, index):
        if index != 0:
            self._marked.add(int(index))

    def _slots_changed(self, old, new):
        mask = stale_blocks(old, new, self._marked, 1 + self.capacity)
        self._marked.clear()
        self.zero_blocks(mask)

    def zero_blocks(self, mask):
        """Zero the ``(h, c)`` rows of the blocks of ``mask`` (bool ``[blocks]``) in both slots of the live actor's actor memory: in place and
        stream-ordered.  Nothing to do while the live actor has no state yet (it is allocated as zeros)."""
        live = self.live
        if getattr(live, "num_envs", None) is None or not bool(mask.any()):
            return
        rows = mask.repeat_interleave(BLOCK)[:live.num_envs]
        if rows.shape[0] != live.num_envs:
            raise ValueError(f"the pool's slot table serves {mask.shape[0]} blocks, the live actor's state has {live.num_envs} rows")
        rows = rows.to(live.state_a[0][0].device).unsqueeze(1)
        for pair in live.state_a:
            for t in pair:
                t.masked_fill_(rows, 0.0)

    def state(self):
        """``PoolBase.state`` and the slot table: which member's weights produced the state of a block is part of a recurrent pool's state."""
        d = super().state()
        if self._slots_host is not None:
            d["slots"] = self._slots_host.clone()
        return d

    def load_state(self, d):
        """``PoolBase.load_state`` (every snapshot counts as overwritten), then the checkpoint's slot table when it fits this pool's: the deal
        zeroes the blocks of the snapshots, whose states the checkpoint does not carry."""
        super().load_state(d)
        if "slots" in d and (self._slots is None or tuple(d["slots"].shape) == tuple(self._slots.shape)):
            self.set_slots(d["slots"])

    # ------------------------------------------------------------------ separate launches (rc -4, wide precision 0, no library)
    def _buffers(self, n):
        live = self.live
        if live.num_envs != n:
            live._allocate(n)
        Ha, na = live.lstm_a.hidden, live.num_actions
        if self._scratch is None or self._scratch[0].shape != (n, Ha):
            z = lambda w: torch.empty(n, w, device=self.device)
            self._scratch = (z(Ha), z(Ha), z(na), z(na))
        self.slot_table(n)
        host = self._slots_host.clamp(0, self.capacity)                     # the kernel's clamp to [0, count)
        env_slot = self._slots.clamp(0, self.capacity).long().repeat_interleave(BLOCK)[:n].unsqueeze(1)
        return host, env_slot

    def step_memory_separate(self, obs, reset=None):
        """What the pooled cell launch computes for this role's actor memory without it: for every member in use one ``lg_lstm_step`` with
        that member's actor memory alone on ALL envs, from the live actor's read slot into scratch, rows selected by block into the write
        slot.  Returns the new ``h`` (the write slot); the caller advances the slots (``advance_slots``)."""
        from .recurrent_actor import lstm_step
        live, n = self.live, obs.shape[0]
        host, env_slot = self._buffers(n)
        h_s, c_s = self._scratch[:2]
        f = live._flip
        h_out, c_out = live.state_a[1 - f]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for k, s in enumerate(sorted(set(host.tolist()))):
            lstm_step(live.lib, self.members[s].lstm_a, None, live._f32(obs), None, live._flags(reset), live.state_a[f], (h_s, c_s), None, None, n, stream)
            rows = env_slot == s
            if k == 0:
                h_out.copy_(h_s); c_out.copy_(c_s)
            else:
                h_out.copy_(torch.where(rows, h_s, h_out)); c_out.copy_(torch.where(rows, c_s, c_out))
        return h_out

    def act_separate(self, h, deterministic):
        """What the pooled actor launch computes for this role without it: for every member in use one ``lg_lstm_actor_act`` on the combined
        ``h`` of ALL envs with the live actor's seed and this step, rows selected by block.  Returns ``(sample, mean, std)``: the first two in
        the live actor's output buffers, ``std`` [n, actions] the rows' members' std.  Counts one step of the live actor's noise stream."""
        live, n = self.live, h.shape[0]
        lib = live.lib
        host, env_slot = self._buffers(n)
        a, mu = self._scratch[2:]
        actions, mean = live.output_buffers(n)
        step, ctr = live.next_step()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        std = torch.empty_like(actions)
        for k, s in enumerate(sorted(set(host.tolist()))):
            member = self.members[s]
            rc = lib.lg_lstm_actor_act(member.fused.handle, h.data_ptr(), a.data_ptr(), mu.data_ptr(), n, live.seed, step, ctr, int(bool(deterministic)), stream)
            if rc != 0:
                raise RuntimeError(f"lg_lstm_actor_act failed ({rc}): {lib.lg_last_error().decode()}")
            rows = env_slot == s
            member_std = member.ac.std.detach().expand(n, -1)
            if k == 0:
                actions.copy_(a); mean.copy_(mu); std.copy_(member_std)
            else:
                actions.copy_(torch.where(rows, a, actions)); mean.copy_(torch.where(rows, mu, mean)); std.copy_(torch.where(rows, member_std, std))
        return actions, mean, std
