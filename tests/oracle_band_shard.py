"""Test adapter for band sharding over gloo: tests/oracle_shard.py's OracleShard with the HIP renderer's render_window signature
(its last argument is a stream, the oracle's a thread count).  Test infrastructure only."""
from oracle_shard import OracleShard


class OracleBandShard(OracleShard):
    def render_window(self, x0, y0, x1, y1, w0, w1, stream=None):
        self.o.render_window(x0, y0, x1, y1, w0, w1, 1)

    def training_stats(self):
        return self.o.training_stats()
