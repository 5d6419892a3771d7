"""Continuous batching over one engine.

The reference serves a JSONL batch as one static batch: every row is stepped (and padded) until the longest
dialogue ends (modeling_asteroid.py:155-169).  Dialogues are independent, so here a finished dialogue leaves its
slot at once, its KV pages return to the engine's page pool, and the next queued one is prefilled into the slot while
the others keep decoding; the weight stream of every step is shared by whatever is resident.  Each dialogue's tokens
are exactly what it would get alone (`Engine.generate` with batch 1 and the same seed): nothing in a row's arithmetic
depends on its neighbours.

Admission is by free KV pages, not by slots alone: the pool (`Engine(kv_pool_pages=...)`) may hold far fewer pages
than `slots x max_seq_len` tokens.  A prompt is admitted when its pages are free with one page of headroom per
resident dialogue (each of them opens a new page every 64 steps); pages for generated tokens are taken as the
dialogues grow.  If the pool still runs dry mid-flight (`mtts_step` -> MTTS_ENOMEM) the dialogue with the fewest
generated rows is evicted and re-queued -- tokens are a function of (prompt, seed), so its re-run reproduces them --
and nothing new is admitted until a resident dialogue has finished (otherwise the evicted prompt would take the freed
pages straight back).

Takes (`run(..., takes=n)`, HF num_return_sequences): when a prompt is admitted its other takes are forked into the
slots free at that moment (`Engine.fork`: the complete prompt pages are shared, one page copied, no prefill), as far as
pages allow; a take that gets no slot then, or is evicted later, is queued as a plain submission with its own row id
and reproduces the same tokens.
"""
from __future__ import annotations

import numpy as np

from . import capi


class ContinuousBatcher:
    def __init__(self, engine, slots, gen_cap, layers=None, do_samples=None, steps_per_poll=16):
        self.eng = engine
        self.slots = int(slots)
        self.gen_cap = int(gen_cap)
        self.steps_per_poll = int(steps_per_poll)
        self.evictions = 0
        self.forks = 0                                                # takes started by Engine.fork (no prefill of their own)
        self._layers, self._do_samples, self._scores, self._topk = layers, do_samples, False, 0
        engine.sched_open(self.slots, self.gen_cap, layers=layers, do_samples=do_samples)

    def run(self, prompts, max_new_tokens, seeds=None, base_seed=0, row_ids=None, takes=1, output_scores=False, adapters=None,
            top_logprobs=None):
        """prompts: list of int64 [T_i,8] delay-shifted prompts (no padding); max_new_tokens: int or list
        (HF semantics: max_length = T_i + max_new).  seeds: one Philox key per dialogue (default base_seed + i, so
        that concurrent dialogues draw from different streams).  Returns a list of int64 [T_i-7+G_i, 8] in
        submission order.  row_ids: Philox row id per dialogue (default 0): with one shared seed and row_ids = the
        dialogues' positions in a batch they draw what that static batch's rows draw.
        takes: sampled takes per prompt; take j of prompt i draws with seeds[i] and row id row_ids[i] * takes + j (the
        row of the repeat-interleaved batch), and the result list holds len(prompts) * takes entries, take j of prompt
        i at i * takes + j.
        output_scores: returns (results, scores), scores[k] float32 [G_k, 8] = the log-probabilities of job k's generated
        rows (Engine.generate: lp).  They are a function of (prompt, seed, row id) like the tokens: an evicted and re-run
        dialogue, a forked take and a queued take all reproduce them.
        adapters: one bank index per prompt (Engine.load_bank_adapter; None / -1: none).  It is kept with the job: an
        evicted and re-queued dialogue and a queued take are submitted with it again, a forked take inherits it.
        top_logprobs=k (1..16): returns (results, scores or None, (logprobs, top_ids, top_logprobs)), each of the three a
        per-job list like scores: float32 [G_k, 8], int32 [G_k, 8, k], float32 [G_k, 8, k] (Engine.generate: top_logprobs),
        reproduced by re-runs, forks and queued takes like the scores.  Without the argument the return value is as above."""
        takes = int(takes)
        if takes < 1:
            raise ValueError(f"takes must be >= 1 (got {takes})")
        topk = 0 if top_logprobs is None else int(top_logprobs)
        if bool(output_scores) != self._scores or topk != self._topk:  # the switches are read when the scheduler opens
            self._scores, self._topk = bool(output_scores), topk
            self.eng.sched_open(self.slots, self.gen_cap, layers=self._layers, do_samples=self._do_samples,
                                output_scores=self._scores, top_logprobs=self._topk)
        n = len(prompts)
        mnt = [max_new_tokens] * n if np.isscalar(max_new_tokens) else list(max_new_tokens)
        seeds = list(seeds) if seeds is not None else [int(base_seed) + i for i in range(n)]
        row_ids = [0] * n if row_ids is None else [int(r) for r in row_ids]
        adapters = [-1] * n if adapters is None else [-1 if a is None else int(a) for a in adapters]
        if len(adapters) != n:
            raise ValueError(f"adapters has {len(adapters)} entries, there are {n} prompts")
        # jobs k = i * takes + j; a queued job forks the prompt's other takes when it is admitted only if it is take 0 on
        # its first admission
        prompts = [prompts[k // takes] for k in range(n * takes)]
        mnt = [mnt[k // takes] for k in range(n * takes)]
        seeds = [seeds[k // takes] for k in range(n * takes)]
        row_ids = [row_ids[k // takes] * takes + k % takes for k in range(n * takes)]
        adapters = [adapters[k // takes] for k in range(n * takes)]
        forks = set(range(0, n * takes, takes)) if takes > 1 else set()
        n *= takes
        results = [None] * n
        scores = [None] * n
        tops = ([None] * n, [None] * n, [None] * n)
        owner = [-1] * self.slots
        queue = list(range(n)) if takes == 1 else list(range(0, n, takes))
        steps = 0
        hold = False                                                  # after an eviction: wait for a dialogue to finish
        polls = 0
        while queue or any(o >= 0 for o in owner):
            polls += 1
            if polls > 1_000_000:
                raise capi.MttsError("continuous batcher made no progress (scheduling bug)")
            for s in range(self.slots):                               # refill free slots while pages last
                if owner[s] < 0 and queue and not hold:
                    i = queue[0]
                    ids = np.asarray(prompts[i], dtype=np.int64)
                    live = sum(1 for o in owner if o >= 0)
                    if live and self.eng.kv_pool_state()[1] < (ids.shape[0] - 7 + 64) // 64 + live + 1:
                        break                                         # not enough headroom next to the residents
                    try:
                        self.eng.submit(s, ids, ids.shape[0] + int(mnt[i]), seed=int(seeds[i]), row_id=row_ids[i],
                                        adapter=adapters[i])
                    except capi.MttsError as err:
                        if err.code != capi.ENOMEM:
                            raise
                        if not any(o >= 0 for o in owner):
                            raise                                     # does not fit an empty pool: not a scheduling matter
                        break                                         # wait for a resident dialogue to finish
                    queue.pop(0)
                    owner[s] = i
                    if i in forks:
                        forks.discard(i)
                        self._fork_takes(s, i, takes, ids.shape[0], owner, queue, seeds, row_ids)
            try:
                self.eng.step(self.steps_per_poll)
                steps += self.steps_per_poll
            except capi.MttsError as err:
                if err.code != capi.ENOMEM:
                    raise
                st = self.eng.slot_states()                           # also returns the pages of finished slots
                live = [s for s in range(self.slots) if owner[s] >= 0 and st[s, 0]]
                if len(live) == sum(1 for s in range(self.slots) if owner[s] >= 0):
                    if len(live) <= 1:
                        raise                                         # one dialogue alone exhausts the pool
                    victim = min(live, key=lambda s: (st[s, 2], -s))  # least work lost
                    self.eng.evict(victim)
                    queue.insert(0, owner[victim])
                    owner[victim] = -1
                    self.evictions += 1
                    hold = True
            st = self.eng.slot_states()
            for s in range(self.slots):
                if owner[s] >= 0 and not st[s, 0]:                    # left the batch: collect
                    i = owner[s]
                    rows = self.eng.slot_read(s, self.gen_cap)
                    if self._scores:
                        scores[i] = self.eng.slot_read_scores(s, self.gen_cap)
                    if self._topk:
                        tops[0][i], tops[1][i], tops[2][i] = self.eng.slot_read_top_logprobs(s, self.gen_cap)
                    ids = np.asarray(prompts[i], dtype=np.int64)
                    results[i] = np.concatenate([ids[:ids.shape[0] - 7], rows], axis=0)
                    owner[s] = -1
                    hold = False
        self.engine_steps = steps
        if top_logprobs is not None:
            return results, (scores if self._scores else None), tops
        return (results, scores) if self._scores else results

    def _fork_takes(self, s, i, takes, T, owner, queue, seeds, row_ids):
        """Take 0 of a prompt (job i) has just been submitted to slot s: fork takes 1.. into free slots while a page for
        each take's copy of the last prompt page stays free next to the residents' headroom; the rest are queued (at the
        front, in take order) as plain submissions."""
        left = list(range(i + 1, i + takes))
        own = 1 if (T - 7) % 64 else 0                                # private pages a take needs now
        for d in range(self.slots):
            if not left:
                break
            if owner[d] >= 0:
                continue
            live = sum(1 for o in owner if o >= 0)
            if self.eng.kv_pool_state()[1] < own + live + 1:
                break
            try:
                self.eng.fork(s, d, seed=int(seeds[left[0]]), row_id=row_ids[left[0]])
            except capi.MttsError as err:
                if err.code != capi.ENOMEM:
                    raise
                break
            owner[d] = left.pop(0)
            self.forks += 1
        queue[:0] = left
