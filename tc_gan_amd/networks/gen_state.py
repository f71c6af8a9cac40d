"""Device-side state of a generator's update, owned in one place: `GeneratorParamState` (the parameters of one generator on
the device with their moments, bounds, record buffer and host mirror), `flat_bounds` (clip bounds per element) and
`HostRecord` (pinned buffers a step's record comes back through).  The GAN loop (`networks.cwgan`) and the critic-free
trainers (`networks.moment_matching`) build one `GeneratorParamState` each; nothing here launches an update."""
import numpy as np
import torch

from ..utils import to_device


def flat_bounds(sizes, bounds):
    """(lo, hi) as float32 vectors of sum(sizes) elements: pair i of `bounds` -- scalars, or arrays for bounds per element,
    which the reference clips with numpy broadcasting (wgan.py:244-251) -- broadcast over the sizes[i] elements of its parameter."""
    lo, hi = (np.concatenate([np.broadcast_to(np.asarray(pair[side], dtype='float32').ravel(), (int(size),))
                              for size, pair in zip(sizes, bounds)]) for side in (0, 1))
    return lo, hi


class GeneratorParamState(object):
    """The parameters of one generator on the device, in `get_all_params` order (['V',] 'J', 'D', 'S'): one flat fp32 vector
    `flat` with a view per name (`params`), the flat optimizer moments `m` / `v`, the clip bounds `lo` / `hi` per element, the
    `n + 1` record buffer of the one-launch update (new values, loss) and `mirror`, the host values the device copy
    corresponds to."""

    def __init__(self, gen, param_bounds):
        self.names = [name for name, _ in gen.get_all_params()]
        sizes = [int(np.size(value)) for _, value in gen.get_all_params()]
        self.offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        self.n = int(self.offs[-1])
        self.flat = torch.zeros(self.n, device='cuda', dtype=torch.float32)
        self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.params = {name: self.flat[a:b] for name, (a, b) in zip(self.names, self.ranges())}
        self.lo, self.hi = (to_device(b) for b in flat_bounds(sizes, [param_bounds[name] for name in self.names]))
        self.record = torch.empty(self.n + 1, device='cuda', dtype=torch.float32)
        self.mirror = {}

    def ranges(self):
        """[(first, past-the-last)] of every parameter's elements in the flat vectors, `names` order."""
        return list(zip(self.offs[:-1], self.offs[1:]))

    def upload_changed(self, gen):
        """The device copies are the working values: a parameter is uploaded only when somebody changed the generator's
        attribute since the last `write_back` (wgan.py:218-260)."""
        for name in self.names:
            value = np.asarray(getattr(gen, name))
            cached = self.mirror.get(name)
            if cached is None or cached.shape != value.shape or not np.array_equal(cached, value):
                self.params[name].copy_(to_device(np.ascontiguousarray(value, dtype='float32').ravel()))

    def write_back(self, gen, host):
        """The new values of an update's record `host` (flat, `names` order) into the generator's attributes and the mirror."""
        for name, (a, b) in zip(self.names, self.ranges()):
            new = host[a:b].astype('float64').reshape(np.shape(getattr(gen, name)))
            setattr(gen, name, new)
            self.mirror[name] = new.copy()

    def matches(self, gen):
        """Are the generator's attributes still the values of the last `write_back`?"""
        return all(name in self.mirror and np.array_equal(self.mirror[name], np.asarray(getattr(gen, name)))
                   for name in self.names)

    def in_step(self, updaters, gen_dtype):
        """Can all parameters be updated by one launch?  A float32 generator whose updaters are in step with each other
        (same rule, hyper-parameters and step count: the builders make them that way)."""
        sig = {(u.kind, u.learning_rate, tuple(sorted(u.cfg.items())), tuple(u.reg), u.step)
               for u in (updaters[name] for name in self.names)}
        return len(sig) == 1 and gen_dtype == 'float32'

    def bind_moments(self, updaters):
        """The updaters' moments become views of `m` / `v` (checkpoints read them there); moments restored from a checkpoint
        are taken over."""
        for name, (a, b) in zip(self.names, self.ranges()):
            u, mine = updaters[name], (self.m[a:b], self.v[a:b])
            if u._state is None:
                mine[0].zero_(); mine[1].zero_()
                u._state = mine
            elif u._state[0].data_ptr() != mine[0].data_ptr():
                mine[0].copy_(u._state[0].reshape(-1)); mine[1].copy_(u._state[1].reshape(-1))
                u._state = mine

    def jds_v_slices(self):
        """dict(JDS=the 12 contiguous values of J, D, S[, V=...]) as views of `flat` -- what a forward with device-resident
        parameters reads (`ssn_build_w_devparams_f32`) -- or None when the layout is another one."""
        names, offs = self.names, self.offs
        j = names.index('J')
        if names[j:j + 3] != ['J', 'D', 'S'] or offs[j + 3] - offs[j] != 12:
            return None
        pd = dict(JDS=self.flat[offs[j]:offs[j] + 12])
        if 'V' in names:
            pd['V'] = self.params['V']
        return pd


class HostRecord(object):
    """A ring of `length` pinned host buffers, each with an event: `post(tensor)` queues the asynchronous copy of a small
    fp32 device tensor and returns a ticket, `ticket.wait()` waits for that copy alone (not for later launches) and returns
    the values.  A buffer is read before the ring comes round; pinned memory is allocated on first use and on a size change."""

    class Ticket(object):
        def __init__(self, host, event):
            self.host, self.event = host, event

        def wait(self):
            self.event.synchronize()
            return self.host.numpy().copy()               # (the pinned buffer goes back to the ring)

    def __init__(self, length):
        self.length = length
        self._ring = []
        self._pos = -1

    def post(self, tensor):
        if not self._ring or self._ring[0].host.numel() != tensor.numel():
            self._ring = [self.Ticket(torch.empty(tensor.numel(), dtype=torch.float32, pin_memory=True), torch.cuda.Event())
                          for _ in range(self.length)]
        self._pos = (self._pos + 1) % self.length
        ticket = self._ring[self._pos]
        ticket.host.copy_(tensor, non_blocking=True)
        ticket.event.record()
        return ticket
