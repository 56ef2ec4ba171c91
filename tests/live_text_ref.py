"""A brute-force restatement of `stream.TextPlan`: readiness decided token by token and frame by frame,
with sets instead of counters.  It shares no code with the plan; the tests drive both with the same events.

`dur_of(t, E)` gives the frames of token t when its block was encoded from a prefix of E tokens."""


def schedule(T, c, cap):
    out, first = [], 0
    while first < T:
        n = min(c, T - first)
        out.append((first, n))
        first, c = first + n, min(2 * c, cap)
    return out


class RefText:
    def __init__(self, bt, A, R, r_dec, dec, chunk, cap, flow_frames, over_frames, dur_of):
        self.bt, self.A, self.R, self.r_dec, self.dec = bt, A, R, r_dec, dec
        self.chunk, self.cap, self.ff, self.over = chunk, cap, flow_frames, over_frames
        self.dur_of = dur_of
        self.tokens = set()                    # the tokens that have arrived
        self.closed = False
        self.encoded = {}                      # token -> its frames
        self.blocks = 0
        self.flowed = set()                    # z frames that are flowed
        self.released = 0                      # chunks released
        self.log = []

    def push(self, n):
        assert not self.closed
        base = len(self.tokens)
        self.tokens |= set(range(base, base + n))

    def close(self):
        assert self.tokens
        self.closed = True

    # ---- what exists
    def _frames(self):
        """[token of frame 0, token of frame 1, ...] over the encoded tokens."""
        out = []
        for t in sorted(self.encoded):
            out += [t] * self.encoded[t]
        return out

    def _complete(self):
        return self.closed and all(t in self.encoded for t in self.tokens)

    def tick(self):
        N = len(self.tokens)
        # token blocks, one by one: every token of the block's prefix must exist (the prefix is cut at N once closed)
        while True:
            k = self.blocks
            own = [t for t in range(k * self.bt, (k + 1) * self.bt) if t in self.tokens]
            if self.closed:
                if not own:
                    break
                prefix = [t for t in range(N if self.A is None else (k + 1) * self.bt + self.A) if t in self.tokens]
            else:
                if self.A is None:
                    break
                prefix = list(range((k + 1) * self.bt + self.A))
                if any(t not in self.tokens for t in prefix):
                    break
            E = len(prefix)
            for t in own:
                if t < E:
                    self.encoded[t] = self.dur_of(t, E)
            self.blocks += 1
            self.log.append(("block", k, E))
        frames = self._frames()
        P, complete = len(frames), self._complete()
        # z frame t may be flowed iff z_p frame t + R exists, or nothing will come behind P
        can = [t for t in range(P) if t not in self.flowed and (complete or t + self.R < P)]
        if can and (complete or len(can) >= self.ff):
            assert can == list(range(can[0], can[-1] + 1)) and (can[0] == 0 or can[0] - 1 in self.flowed)
            self.flowed |= set(can)
            self.log.append(("flow", can[0], can[-1] + 1))
        # chunks, one by one
        T = P if complete else None
        first, c = 0, self.chunk
        idx = 0
        while True:
            if complete and first >= T:
                break
            n = min(c, T - first) if complete else c
            if self.dec is None:
                need = range(T) if complete else range(first + n + self.r_dec)
                D = None
            else:
                D = first + n + self.dec
                if complete:
                    D = min(D, T)
                need = range(D)
            if idx >= self.released:
                if any(t not in self.flowed for t in need):
                    break
                over = 0 if D is None else min(self.over, D - first - n)
                self.log.append(("chunk", first, n, D, over))
                self.released += 1
            first, c, idx = first + n, min(2 * c, self.cap), idx + 1
        return self.log

    @property
    def done(self):
        return self._complete() and sum(n for e in self.log if e[0] == "chunk" for n in [e[2]]) == len(self._frames())
