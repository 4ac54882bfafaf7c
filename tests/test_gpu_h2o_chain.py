"""H2O eviction inside the decode engine, end to end against an oracle that evicts too.

A teacher-forced chain per variant: the prompt pass in chunks with `set_h2o(True)`, then one logits-only step per token at
cache positions feeding the device's own argmax; whenever the cache is full, `h2o_evict(..., move_pos=False)`. The
reference is the fp32 CPU oracle (`LlamaOracle`) with its attention wrapped by `tests/h2o_reference.ScoreBook`.

At every eviction the cache bits and the scores are read before and after the call:
 1. the rows the device kept, found per (layer, kv head) by matching V row bytes, are `h2o_reference.select` of the
    device's own scores read before the call, exactly. (Layer 0's V row depends on the token alone and the greedy chain
    repeats tokens: equal V rows are told apart by their score bits, which are asserted to differ; see `_kept_rows`);
 2. the kept V rows and scores are compacted bit for bit; the `n_discard` score rows the compaction frees are zero (the
    compact kernel clears them: the next steps add to them) and the rows beyond the old length are left as they were;
 3. every kept K row is the rotate-back of the device's own stored row by its own distance within
    `kv_shift_reference.MAX_ULP` / `MAX_DIFFERING` (the kernel test's bound), unmoved rows keep their bytes;
 4. the device scores before the call lie within expm1(2 d), d = 2e-2 * max|logit|, of the ScoreBook's (the derivation of
    tests/test_gpu_h2o_engine.py); from the second eviction on these are scores that were compacted and added to again;
 5. the oracle and the ScoreBook then evict the set the DEVICE kept, so the chain cannot fork on a near-tie of two scores.
Every step's logits meet the decode tolerance 2e-3 * max|ref| + 1e-4; the argmax is equal wherever the oracle's top-two
gap exceeds twice that, and at most 2 steps of a chain differ inside it.

fp16 caches: the oracle keeps its own fp32 rows throughout; the device's K rows lie within (1 + moves of the row) fp16
ulps + 2e-3 * max + 1e-4 of them. bf16 / e4m3 caches: teacher-forced through `kv_hook` as in
tests/test_gpu_attention_fullgeom.py — the oracle caches the rows the device stored, the rows it computed itself are
compared at KV_TOL * max + half a storage step, and after an eviction that passed check 3 it adopts the moved K rows.

A chain runs its number of steps and evicts once more if the last step filled the cache, so that the last compaction
is checked too (no step follows it).

The tiny model attends almost evenly, so the lowest scores are mostly the newest rows of the range and the kv heads mostly
agree on them (every variant prints how many neighbouring heads chose differently). A sixth variant, `fp16-d64-spread`,
therefore adds one random fp32 offset to the device's scores (`h2o_scores()` is a view) and to the ScoreBook's before
every eviction: the checks are the same, and every (layer, kv head) drops rows of its own.

Measured on an MI355X (evictions; worst logit error / tolerance; worst relative score error and its bound; worst K ulp
distance; steps excused by the top-two rule):
  fp16-d64         7   0.113   2.6e-04 (bound 1.17e-01)   0 ulp              0
  bf16-d64         3   0.000   5.4e-05 (bound 1.11e-01)   0 ulp              0   (teacher-forced: the logits agree to fp32)
  e4m3-d64         3   0.000   5.3e-05 (bound 1.25e-01)   0 ulp              0   (teacher-forced)
  fp16-d128        3   0.344   5.8e-04 (bound 2.34e-01)   0 ulp              0
  fp16-long        3   0.030   1.9e-04 (bound 1.43e-01)   0 ulp              0
  fp16-d64-spread  3   0.113   6.3e-05 (bound 1.21e-01)   1 ulp (6e-4 of the elements)   0
Cache rows against the oracle's: at most 0.31 of their bound (fp16-d128). Neighbouring kv heads that kept different rows:
1 of 14, 1 of 6, 2 of 6, - (one kv head), 2 of 6, and 6 of 6 with the offset. Every selection differed from the rolling
cache's. With the compact kernel rotating by the destination row in place of the distance, check 3, the cache rows and the
logits fail in every variant; with `select` given n_cached - 1 by the engine, check 1 fails in every variant.
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd.runtime.engine import H2OConfig, build_rope_tables
from tests import h2o_reference as H
from tests import kv_shift_reference as KR
from tests.test_gpu_attention_fullgeom import KV_TOL
from tests.test_gpu_engine import _tiny
from tests.test_gpu_streaming_engine import _fp16_ulp

pytestmark = pytest.mark.gpu

PROMPT = [7, 300, 12, 45, 99, 3]
LONG_PROMPT = np.random.default_rng(17).integers(0, 384, 260).tolist()
SIG_BITS = {"fp16": 11, "bf16": 8, "e4m3": 4}  # significant bits: half a storage step is 2^-bits of the value
VARIANTS = {
    "fp16-d64": dict(kind="fp16", model=dict(max_ctx=32), geometry=(32, 4, 7, 5), prompt=PROMPT, chunk=4, steps=70,
                     evictions=7),
    "bf16-d64": dict(kind="bf16", model=dict(max_ctx=32), geometry=(32, 4, 7, 5), prompt=PROMPT, chunk=4, steps=40,
                     evictions=3),
    "e4m3-d64": dict(kind="e4m3", model=dict(max_ctx=32), geometry=(32, 4, 7, 5), prompt=PROMPT, chunk=4, steps=40,
                     evictions=3),
    "fp16-d128": dict(kind="fp16", model=dict(max_ctx=64, head_dim=128, hidden=512), geometry=(32, 4, 7, 0),
                      prompt=PROMPT, chunk=4, steps=40, evictions=3),
    "fp16-long": dict(kind="fp16", model=dict(max_ctx=320), geometry=(288, 4, 16, 8), prompt=LONG_PROMPT, chunk=100,
                      steps=60, evictions=3),
    # beyond the five above: scores with a known random offset of up to 16 per row, which outweighs the scores of the range
    # (below 6 here): every (layer, kv head) then drops what is close to a draw of its own of 7 rows out of 23
    "fp16-d64-spread": dict(kind="fp16", model=dict(max_ctx=32), geometry=(32, 4, 7, 5), prompt=PROMPT, chunk=4, steps=40,
                            evictions=3, spread=16.0),
}


def _bits(eng, which):
    return KR.bits_of(eng.kv_cache(which)[0])  # [layers, max_ctx, kv heads, D]


def _kept_rows(v0, s0, v1, s1, m):
    """One (layer, kv head): V row bits before [n, D] and after, score bits before [n] and after -> the source row of each
    of the first m rows after (-1 where a row after is none of the rows before), and how many needed their score.
    A row is known by its V bytes. Layer 0's V row is a function of the token alone, so a chain that repeats a token
    holds equal V rows there (and their K rows are equal once rotated to the same row): those are told apart by their
    score bits, which must then differ — the condition on the inputs that makes the kept set readable at all."""
    rows = {}
    for i, row in enumerate(v0):
        rows.setdefault(row.tobytes(), []).append(i)
    src, by_score = [], 0
    for j in range(m):
        cand = rows.get(v1[j].tobytes(), [])
        if len(cand) > 1:
            assert len({s0[i].tobytes() for i in cand}) == len(cand), "equal V rows with equal scores cannot be told apart"
            cand, by_score = [i for i in cand if s0[i].tobytes() == s1[j].tobytes()], by_score + 1
        src.append(cand[0] if len(cand) == 1 else -1)
    return np.array(src), by_score


class _Unreadable(Exception):
    """an eviction after which the kept rows cannot be identified"""


def _run_chain(name):
    v = VARIANTS[name]
    tokens = []
    kind, forced = v["kind"], v["kind"] != "fp16"
    eng, oracle, cfg = _tiny(128, False, "fp16", seed=3, kv_dtype=KR.TORCH_DTYPE[kind], **v["model"])
    ctx, n_keep, n_discard, recent = v["geometry"]
    layers, KV, D, max_ctx = cfg["layers"], cfg["kv_heads"], cfg["head_dim"], eng.cfg.max_ctx
    cos, sin = (t.numpy().astype(np.float64) for t in build_rope_tables(max_ctx, D, cfg["theta"], "cpu"))
    rec = dict(name=name, eng=eng, evictions=0, kept_wrong=[], copy_wrong=[], tail_wrong=[], k_ulp=0, k_differing=0.0,
               k_unmoved_wrong=[], score_rel=0.0, score_bound=0.0, score_wrong=[], logit_ratio=0.0, logit_wrong=[],
               argmax_wrong=[], excused=0, stopped=None, rows_ratio=0.0, rows_wrong=[], heads_apart=0, heads_compared=0,
               not_rolling=0, by_score=0)
    dev = {}

    def read_device():
        for w in "kv":
            dev[w] = KR.decode(_bits(eng, w), kind).astype(np.float32)

    def hook(li, start, k, v_):  # teacher forcing: cache what the device stored, compare what the oracle computed
        s0, n = int(np.asarray(start).ravel()[0]), k.shape[0]
        for w, mine in (("k", k), ("v", v_)):
            err = np.abs(dev[w][li, s0:s0 + n] - mine)
            ratio = float(((err - 2.0 ** -SIG_BITS[kind] * np.abs(mine)) / (KV_TOL * np.abs(mine).max())).max())
            rec["rows_ratio"] = max(rec["rows_ratio"], ratio)
            if ratio > 1:
                rec["rows_wrong"].append((w, li, s0, ratio))
        return dev["k"][li, s0:s0 + n].copy(), dev["v"][li, s0:s0 + n].copy()

    def judge(got, ref, where, tol_rel, tol_abs):
        tol = tol_rel * float(np.abs(ref).max()) + tol_abs
        ratio = float(np.abs(got - ref).max()) / tol
        rec["logit_ratio"] = max(rec["logit_ratio"], ratio) if where != "prompt" else rec["logit_ratio"]
        if ratio > 1:
            rec["logit_wrong"].append((where, ratio))
        if int(got.argmax()) != int(ref.argmax()):
            top = np.sort(ref)[-2:]
            if top[1] - top[0] > 2 * tol:
                rec["argmax_wrong"].append(where)
            else:
                rec["excused"] += 1

    rng = np.random.default_rng(23)

    def spread(book, p):
        """with `spread`: the same random fp32 offset on the device's and the ScoreBook's scores of the cached rows"""
        if v.get("spread"):
            r = (rng.random((layers, KV, p)) * v["spread"]).astype(np.float32)
            eng.h2o_scores()[..., :p].add_(torch.from_numpy(r).to(eng.device))
            book.score[..., :p] += r

    moves = np.zeros((layers, KV, max_ctx), np.int64)  # times the K row now in a cache row was re-rounded by a move

    def evict(book, p):
        assert p == ctx
        m, e = ctx - n_discard, rec["evictions"]
        k0, v0, s0 = _bits(eng, "k"), _bits(eng, "v"), eng.h2o_scores().cpu().numpy()
        eng.h2o_evict(n_keep, n_discard, recent, ctx, move_pos=False)
        k1, v1, s1 = _bits(eng, "k"), _bits(eng, "v"), eng.h2o_scores().cpu().numpy()
        # 4. the scores the selection read, against the oracle's
        d = 2e-2 * book.logit
        rel = np.abs(s0[..., :ctx] - book.score[..., :ctx]) / book.score[..., :ctx]
        rec["score_rel"] = max(rec["score_rel"], float(rel.max()))
        rec["score_bound"] = max(rec["score_bound"], float(np.expm1(2 * d)))
        if not (rel <= np.expm1(2 * d)).all():
            rec["score_wrong"].append((e, float(rel.max()), float(np.expm1(2 * d))))
        kept = np.zeros((layers, KV, ctx), bool)
        k_ok = True
        for l in range(layers):
            want = H.select(s0[l], n_keep, n_discard, recent, ctx)
            for h in range(KV):
                # 1. which rows the device kept
                src, by_score = _kept_rows(v0[l, :ctx, h], s0[l, h, :ctx], v1[l, :m, h], s1[l, h, :m], m)
                rec["by_score"] += by_score
                if (src < 0).any() or (np.diff(src) <= 0).any():  # not rows from before, in order: nothing to follow
                    rec["kept_wrong"].append((e, l, h, "rows after <- rows before", src.tolist()))
                    raise _Unreadable("eviction %d, layer %d, kv head %d" % (e, l, h))
                kept[l, h, src] = True
                if not np.array_equal(kept[l, h], want[h]):
                    rec["kept_wrong"].append((e, l, h, np.flatnonzero(~kept[l, h]).tolist(), np.flatnonzero(~want[h]).tolist()))
                rec["not_rolling"] += int(kept[l, h, n_keep:n_keep + n_discard].any())
                # 2. V (by construction of src) and the scores, bit for bit; the freed score rows zero, the rest left
                to = np.arange(m)
                if not np.array_equal(s1[l, h, :m].view(np.uint32), s0[l, h, src].view(np.uint32)):
                    rec["copy_wrong"].append((e, l, h))
                left = np.array_equal(s1[l, h, ctx:].view(np.uint32), s0[l, h, ctx:].view(np.uint32))  # (never written: 0)
                if s1[l, h, m:ctx].view(np.uint32).any() or not left or s1[l, h, ctx:].any():
                    rec["tail_wrong"].append((e, l, h))
                # 3. K: the kernel test's reference on the device's own stored rows
                a, b = KR.decode(k0[l, src, h, :D // 2], kind), KR.decode(k0[l, src, h, D // 2:], kind)
                ra, rb = KR.rotate_back(a, b, cos[src - to], sin[src - to])
                dist = KR.ulp_distance(k1[l, to, h], KR.encode(np.concatenate([ra, rb], -1), kind), kind)
                worst, differing = int(dist.max()), float((dist != 0).mean())
                rec["k_ulp"], rec["k_differing"] = max(rec["k_ulp"], worst), max(rec["k_differing"], differing)
                k_ok = k_ok and worst <= KR.MAX_ULP and differing <= KR.MAX_DIFFERING
                if not np.array_equal(k1[l, to[src == to], h], k0[l, src[src == to], h]):
                    rec["k_unmoved_wrong"].append((e, l, h))
                    k_ok = False
                moves[l, h, :m] = moves[l, h, src] + (src != to)
                moves[l, h, m:] = 0
            rec["heads_compared"] += KV - 1
            rec["heads_apart"] += sum(int((kept[l, h] != kept[l, h - 1]).any()) for h in range(1, KV))
        # 5. the oracle follows the device's choice
        H.evict(oracle, kept)
        book.gather(kept)
        if forced:
            read_device()
            if k_ok:
                for l in range(layers):
                    oracle.k[l] = dev["k"][l, :m].copy()
        else:
            k_dev = KR.decode(k1, kind)
            for l in range(layers):
                ok = oracle.k[l]
                bound = (1 + moves[l, :, :m].T[:, :, None]) * _fp16_ulp(ok) + 2e-3 * np.abs(ok).max() + 1e-4
                ratio = float((np.abs(k_dev[l, :m] - ok) / bound).max())
                rec["rows_ratio"] = max(rec["rows_ratio"], ratio)
                if ratio > 1:
                    rec["rows_wrong"].append(("k", l, e, ratio))
        rec["evictions"] += 1
        return m

    prompt, chunk = v["prompt"], v["chunk"]
    eng.launch = "eager"
    eng.clear_status()
    eng.set_fuse_attn(False)
    eng.set_h2o(True)
    eng.h2o_reset()
    oracle.reset()
    oracle.kv_hook = hook if forced else None
    try:
        with H.ScoreBook(layers, cfg["heads"], KV, D, max_ctx) as book:
            assert len(range(0, len(prompt), chunk)) >= 2
            for s in range(0, len(prompt), chunk):
                got = eng.prefill(prompt[s:s + chunk], start_pos=s, greedy=False)[0].cpu().numpy()
            read_device()
            for s in range(0, len(prompt), chunk):
                ref = oracle.forward_prompt(prompt[s:s + chunk], s)
            judge(got, ref, "prompt", 1e-2, 0.0)  # (the prompt pass: fp16 operands)
            tokens += [int(got.argmax())]
            p = len(prompt)
            for i in range(v["steps"]):
                if p == ctx:
                    spread(book, p)
                    p = evict(book, p)
                eng.token.fill_(tokens[-1])
                eng.pos.fill_(p)
                eng.step(greedy=False)
                got = eng.logits.cpu().numpy()
                if forced:
                    read_device()
                judge(got, oracle.forward_token(tokens[-1], p), (i, p, rec["evictions"]), 2e-3, 1e-4)
                tokens.append(int(got.argmax()))
                p += 1
            if p == ctx:
                spread(book, p)
                evict(book, p)
    except _Unreadable as stop:  # check 1 has failed; the chain ends here and the tests read what it recorded
        rec["stopped"] = str(stop)
    finally:
        rec["tokens"], rec["status"] = tokens, eng.status()
        oracle.kv_hook = None
        oracle.reset()
        eng.set_h2o(False)
        eng.set_fuse_attn(True)
    print("%s: evictions %d, worst logit error %.3f of the tolerance, worst relative score error %.3e (bound %.3e), "
          "worst K ulp distance %d (differing %.2e), steps excused by the top-two rule %d; cache rows vs the oracle's %.3f "
          "of their bound; %d of %d neighbouring kv heads kept different rows, %d of %d selections differ from the rolling cache's, "
          "%d kept rows were told apart by their score"
          % (name, rec["evictions"], rec["logit_ratio"], rec["score_rel"], rec["score_bound"], rec["k_ulp"], rec["k_differing"],
             rec["excused"], rec["rows_ratio"], rec["heads_apart"], rec["heads_compared"], rec["not_rolling"],
             rec["evictions"] * layers * KV, rec["by_score"]))
    return rec


_CHAINS = {}


def _chain(name):
    """the chain of one variant, run once per module"""
    if name not in _CHAINS:
        try:
            _CHAINS[name] = _run_chain(name)
        except BaseException as exc:  # noqa: B036 (kept for the tests that follow: they fail the same way, at once)
            _CHAINS[name] = exc
    if isinstance(_CHAINS[name], BaseException):
        raise _CHAINS[name]
    return _CHAINS[name]


@pytest.fixture(scope="module", params=list(VARIANTS))
def chain(request):
    return _chain(request.param)


def test_the_chain_evicts_on_schedule_and_ends_clean(chain):
    v = VARIANTS[chain["name"]]
    assert chain["stopped"] is None, chain["stopped"]
    assert chain["evictions"] == v["evictions"] and len(chain["tokens"]) == v["steps"] + 1 and chain["status"] == 0
    assert len(set(chain["tokens"])) > 4
    assert chain["not_rolling"] > 0  # H2O chose: not the oldest rows every time
    if v.get("spread"):
        assert chain["heads_apart"] == chain["heads_compared"] > 0  # and every kv head for itself


def test_the_device_keeps_what_select_picks_from_its_own_scores(chain):
    assert not chain["kept_wrong"], chain["kept_wrong"][:3]


def test_v_and_scores_are_compacted_bit_for_bit_and_the_freed_scores_are_zero(chain):
    assert not chain["copy_wrong"] and not chain["tail_wrong"], (chain["copy_wrong"][:3], chain["tail_wrong"][:3])


def test_moved_k_rows_are_rotated_back_by_their_own_distance(chain):
    assert chain["k_ulp"] <= KR.MAX_ULP and chain["k_differing"] <= KR.MAX_DIFFERING, (chain["k_ulp"], chain["k_differing"])
    assert not chain["k_unmoved_wrong"], chain["k_unmoved_wrong"][:3]


def test_scores_follow_the_oracles_through_compactions(chain):
    assert 0 < chain["score_bound"] and not chain["score_wrong"], chain["score_wrong"][:3]


def test_cache_rows_follow_the_oracles(chain):
    assert not chain["rows_wrong"], chain["rows_wrong"][:3]


def test_every_steps_logits_follow_the_evicting_oracle(chain):
    assert not chain["logit_wrong"], chain["logit_wrong"][:3]
    assert not chain["argmax_wrong"], chain["argmax_wrong"][:3]
    assert chain["excused"] <= 2, chain["excused"]


@pytest.mark.parametrize("launch,burst", [("graph", 16), ("graph", 5), ("eager", 16), ("eager", 5)])
def test_generate_returns_the_chains_tokens(launch, burst):
    rec = _chain("fp16-d64")
    eng = rec["eng"]
    eng.launch = launch
    eng.captured = False
    eng.clear_status()
    try:
        out = eng.generate(PROMPT, 70, burst=burst, streaming=H2OConfig(32, 4, 7, recent=5))
    finally:
        eng.launch = "eager"
    assert out == rec["tokens"][:70]
    assert eng.status() == 0 and eng.discarded() == 0 and not eng.h2o_installed
