"""Derived copies of a fused chain's weights and the protocol that keeps them current: who writes a form, who stamps it,
who checks it, what a graph capture does - DESIGN.md 4.4.  Nothing here needs a GPU."""
from collections import namedtuple
from contextlib import contextmanager


class WeightForm:
    """One derived copy: alloc() makes its buffer on first use, pack(stream_of) launches what fills it from the weights,
    `holds` is the weights token (FlatArena.weights_token) it was filled for.  A None token is never current."""

    def __init__(self, alloc, pack):
        self._alloc, self._launch = alloc, pack
        self.buffer = self.holds = None

    def allocate(self):
        if self.buffer is None:
            self.buffer = self._alloc()
        return self.buffer

    def pack(self, stream_of):
        self._launch(stream_of)

    def current(self, token):
        return token is not None and self.holds == token

    def mark(self, token):
        self.holds = token

    def invalidate(self):
        self.holds = None

    def ensure(self, token, stream_of):
        if not self.current(token):
            self.pack(stream_of)
            self.holds = token


class PlanesForm(WeightForm):
    """The fp16 weight planes of both directions in one buffer: pack(stream_of, direction) -> that direction's view
    (0 forward operand, 1 backward, 2 both = the whole buffer); `holds` speaks for BOTH directions.
    fresh: (rows, token) of the training forward that left the backward planes: the backward of those rows and weights
    takes them, any other launch drops them.  packed_once: the whole buffer (its zero padding) has been packed."""

    def __init__(self, alloc, pack, jobs):
        super().__init__(alloc, pack)
        self._two_launches = jobs > 8                 # more jobs than one pack launch carries
        self.fresh, self.packed_once = None, False

    def pack(self, stream_of, direction=2):
        if direction == 2 and self._two_launches:
            self._launch(0, stream_of)
            self._launch(1, stream_of)
            return self.allocate()
        return self._launch(direction, stream_of)

    def pack_once(self, token, stream_of):
        if not self.packed_once:
            self.pack(stream_of)
            self.packed_once, self.holds = True, token

    def take_fresh(self, rows, token):
        fresh, self.fresh = self.fresh, None
        return fresh is not None and fresh == (rows, token)

    def drop_fresh(self):
        self.fresh = None

    def invalidate(self):
        self.holds = self.fresh = None


# what ops.MlpChain.cache_state() records: both forms' `holds`, PlanesForm.fresh / .packed_once, the chain's products mode
ChainSnapshot = namedtuple('ChainSnapshot', 'planes frags fresh packed_once products')


# A fused chain (ops.MlpChain) that an agent's captured graphs read.  launches: [(rows, kind), ...] run on it (MlpChain.
# forms_read); arena: the flat parameters its weights live in.  actor: the update graphs read it too, and its fragments are
# packed behind every optimiser step.  planes: brought up to date in front of a replay - False for the actor's chains
# unless the Adam launch writes them (`adam_writes_planes`): their graphs pack the planes themselves.
_ChainForms = namedtuple('_ChainForms', 'chain launches arena actor planes', defaults=(False, True))


class ChainFormSet(list):
    """The chains an agent's graphs read, in the order their forms are brought up to date (forms_read keeps its answers)."""

    def lean_chain(self):
        """The first actor chain that reads fragments (their pack launch follows every optimiser step), or None."""
        return next((f.chain for f in self if f.actor and f.chain.forms_read(f.launches)[0]), None)

    def adam_pack_chain(self):
        """The first actor chain that reads planes the Adam launch writes (`adam_writes_planes`), or None."""
        return next((f.chain for f in self if f.actor and f.planes and f.chain.forms_read(f.launches)[1]), None)

    def before_replay(self, rollout=False):
        """A captured graph holds no pack launch: pack what is stale.  Update graphs read the actor's chains, rollout all."""
        for f in self:
            if rollout or f.actor:
                frags, planes = f.chain.forms_read(f.launches)
                token = f.chain.weights_token()
                if planes and f.planes:
                    f.chain.planes.ensure(token, f.arena)
                if frags:
                    f.chain.frags.ensure(token, f.arena)

    def after_step(self, optimizer, packed=False):
        """Stamps the Adam-written planes; packs the fragments - or, behind a replayed graph, which did (packed), stamps."""
        token = optimizer.weights_token()
        if self.adam_pack_chain() is not None:
            self.adam_pack_chain().planes.mark(token)
        lean = self.lean_chain()
        if lean is not None:
            if not packed:
                lean.frags.pack(optimizer.flat_params)
            lean.frags.mark(token)

    @contextmanager
    def captured(self):
        """Around a graph capture, failed or not: its pack launches were recorded, not run - the stamps go back."""
        states = [(f.chain, f.chain.cache_state()) for f in self]
        try:
            yield
        finally:
            for chain, state in states:
                chain.restore_cache_state(state)

    def set_products(self, mode):
        for f in self:
            f.chain.products = mode
