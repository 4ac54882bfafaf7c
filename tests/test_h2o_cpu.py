"""H2O eviction, the parts that need no GPU: `H2OConfig`'s checks, and the request drivers over the scripted engine of
tests/test_request_driver_cpu.py: an H2O request runs the rolling cache's schedule with evictions in place of shifts."""
import pytest

from intel_extension_for_transformers_amd.runtime import request
from intel_extension_for_transformers_amd.runtime.streaming import H2OConfig, StreamingConfig, h2o_from_keywords
from tests.test_request_driver_cpu import PROMPT, ScriptedEngine


def test_h2o_config_resolves_like_streaming_plus_recent():
    assert H2OConfig(32, 4, 7, 5).resolve(64, 10) == (32, 4, 7, 5)
    assert H2OConfig(32, 4, 14, 14).resolve(32, 6) == (32, 4, 14, 14)  # the rolling cache's own geometry
    assert H2OConfig(64).resolve(64) == (64, 4, 30, 15)                # half dropped, half of the rest recent
    assert H2OConfig(32, 4, 7, 0.25).resolve(64) == (32, 4, 7, 8)      # recent as a ratio of ctx_size
    assert H2OConfig(100, heavy_ratio=0.2, recent_ratio=0.2).resolve(128) == (100, 4, 56, 20)
    assert H2OConfig(32, 4, 7, 5).resolve(64)[:3] == StreamingConfig(32, 4, 7).resolve(64)
    for cfg, max_ctx, n in [(H2OConfig(32, 4, 7, -2), 64, 1),           # recent < 0
                            (H2OConfig(32, 4, 14, 15), 64, 1),          # n_keep + n_discard + recent > ctx_size
                            (H2OConfig(32, 4, 0, 5), 64, 1),            # the rolling cache's rules still hold
                            (H2OConfig(128, 4, 7, 5), 64, 1),
                            (H2OConfig(32, 4, 7, 5), 64, 32),
                            (H2OConfig(32, heavy_ratio=0.6, recent_ratio=0.6), 64, 1)]:
        with pytest.raises(ValueError, match="QBits:"):
            cfg.resolve(max_ctx, n)
    with pytest.raises(ValueError, match="QBits:"):
        H2OConfig(32, heavy_ratio=0.5)
    assert h2o_from_keywords() is None and h2o_from_keywords(ctx_size=32) is None
    assert h2o_from_keywords(dict(ctx_size=32, recent=5)).resolve(64) == (32, 4, 14, 5)
    assert h2o_from_keywords(recent=3, ctx_size=16).resolve(64) == (16, 4, 6, 3)


class _H2OEngine(ScriptedEngine):
    """the scripted engine of the driver tests with H2O's three calls recorded"""

    def set_h2o(self, on=True):
        self.calls.append(("h2o", on))

    def h2o_reset(self):
        self.calls.append(("h2o_reset",))

    def h2o_evict(self, n_keep, n_discard, recent, n_cached, move_pos=True):
        self.evictions = getattr(self, "evictions", []) + [(n_keep, n_discard, recent, n_cached, move_pos)]
        self.kv_shift(n_keep, n_discard, n_cached, move_pos=move_pos)  # (the position follows as in a shift)


@pytest.mark.parametrize("driver", ["chained", "host_fed"])
def test_a_request_with_an_h2o_config_evicts_where_the_rolling_cache_shifts(driver):
    cfg, rolling = H2OConfig(32, 4, 7, 5), StreamingConfig(32, 4, 7)
    run = {"chained": lambda e, s: request.generate(e, PROMPT, 60, burst=5, streaming=s),
           "host_fed": lambda e, s: sum(request.iter_sampled(e, PROMPT, 60, request.DeviceSampler(), burst=5, streaming=s), [])}[driver]
    eng, plain = _H2OEngine(), ScriptedEngine()
    assert run(eng, cfg) == run(plain, rolling)
    assert eng.plan() == plain.plan() and len(plain.shifts) > 2  # the same schedule ...
    assert eng.evictions == [(4, 7, 5, 32, driver == "chained")] * len(plain.shifts)  # ... answered by evictions
    h2o = [c for c in eng.calls if c[0].startswith("h2o")]
    assert h2o == [("h2o", True), ("h2o_reset",), ("h2o", False)] and eng.calls[-1] == ("h2o", False)
    assert not any(c[0].startswith("h2o") for c in plain.calls)
    failing = _H2OEngine(fail_after=3)  # a request that dies leaves H2O off
    with pytest.raises(RuntimeError, match="scripted failure"):
        run(failing, cfg)
    assert [c for c in failing.calls if c[0] == "h2o"] == [("h2o", True), ("h2o", False)]
