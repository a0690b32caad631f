"""Hidden activation of the MNIST MLP (784 -> 100 act -> 10): the definition, on the host.

The reference model's hidden layer is a sigmoid (worker.py:47-49).  ``--activation`` / the
``activation=`` argument of the fused step, the evaluation kernel and the trainer choose among

* ``sigmoid`` (id 0, the default and the reference's): ``h = 1 / (1 + exp(-z))``,
  ``dh/dz = h (1 - h)``;
* ``relu`` (id 1): ``h = max(z, 0)``, ``dh/dz = 1`` where ``h > 0`` and else 0 -- 0 at ``z == 0``,
  and ``z = -0`` gives ``h = +0`` (``tf.nn.relu`` and its gradient);
* ``tanh`` (id 2): ``h = tanh(z)``, ``dh/dz = 1 - h * h``.

Every derivative is a function of ``h`` alone, which is what the kernels' lanes hold: the head
launch (``csrc/kernels/common.h``: ``hidden_act`` / ``hidden_act_bwd``) takes no new load and
the workspace does not change.  With dropout the derivative uses the undropped ``h``:
``hbuf`` and the logits take ``h * mask`` and ``dz1 = dh * mask * act'(h)``.

The ids are the kernels' ``HACT_*``.  Initialisation stays the reference's for every activation
and a checkpoint does not record the activation: an evaluation or a restored run must be told
the one the parameters were trained with.
"""
from __future__ import annotations

NAMES = ("sigmoid", "relu", "tanh")
IDS = {"sigmoid": 0, "relu": 1, "tanh": 2}
DEFAULT = "sigmoid"


def check(name):
    """``name`` as one of ``NAMES`` (``None``: the default), else ValueError."""
    if name is None:
        return DEFAULT
    if not isinstance(name, str) or name not in IDS:
        raise ValueError("unknown hidden activation %r (one of: %s)" % (name, ", ".join(NAMES)))
    return name


def act_id(name):
    """The kernels' id of ``name`` (validated)."""
    return IDS[check(name)]


def forward(z, name):
    """``h(z)`` in ``z``'s dtype (float64 in: the float64 definition)."""
    import torch

    name = check(name)
    if name == "relu":
        # (a select, not a max: -0 and NaN give +0, as the kernels' do)
        return torch.where(z > 0, z, torch.zeros_like(z))
    if name == "tanh":
        return torch.tanh(z)
    return torch.sigmoid(z)


def derivative(h, name):
    """``dh/dz`` as a function of ``h`` (the undropped activation)."""
    name = check(name)
    if name == "relu":
        return (h > 0).to(h.dtype)
    if name == "tanh":
        return 1 - h * h
    return h * (1 - h)


def from_flags(flags, allowed=NAMES, what=None):
    """The validated ``--activation`` of ``flags`` (a flags object without it: the default).
    ``allowed``: the names the caller's path has; another valid name is refused with ``what``
    (the path) in the message."""
    name = getattr(flags, "activation", None) or DEFAULT
    try:
        name = check(name)
    except ValueError as e:
        raise ValueError("--activation: %s" % e)
    if name not in allowed:
        raise ValueError("--activation %s: %s has no %s variant (it supports: %s); all of %s are "
                         "supported by --strategy mirrored --model mlp and --job_name eval"
                         % (name, what or "this path", name, ", ".join(allowed),
                            ", ".join(NAMES)))
    return name


def refuse(flags, what):
    """A trainer without the MLP's hidden layer refuses a non-default ``--activation``."""
    from_flags(flags, allowed=(DEFAULT,), what=what)
