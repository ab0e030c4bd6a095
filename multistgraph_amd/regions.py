"""Region maps: groups of nodes (census tracts) whose totals are forecast, banded and scored (matgcn_groups,
include/matgcn.h; ops.group_sums / ops.group_label_sums).

A map is a CSR list over groups: groups may overlap, nest, be empty or leave nodes out, and a member list is added in the
order it is given.  The map is validated here, on the host, once; the kernels only clamp an index into the row.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib


class RegionMap:
    """``groups``: one index list per region (overlap allowed, order kept), or ``labels``: one region label per node
    (a partition: label g >= 0 puts the node into region g, a negative label into none; members ascending).
    ``weights``: None (every member counts 1), "mean" (1 / |g| per member: the region's average), one list per group
    matching ``groups``, or - with ``labels`` - one weight per node.  ``names``: one string per region."""

    def __init__(self, num_nodes: int, groups: Optional[Sequence[Sequence[int]]] = None,
                 labels: Optional[Sequence[int]] = None, weights=None, names: Optional[Sequence[str]] = None):
        self.num_nodes = int(num_nodes)
        if self.num_nodes < 1:
            raise ValueError("num_nodes must be >= 1, got %d" % self.num_nodes)
        if (groups is None) == (labels is None):
            raise ValueError("give exactly one of groups= (index lists) and labels= (one label per node)")
        node_weights = None
        if labels is not None:
            labels = [int(v) for v in labels]
            if len(labels) != self.num_nodes:
                raise ValueError("labels has %d entries, expected one per node (%d)" % (len(labels), self.num_nodes))
            n_groups = max(labels) + 1 if labels else 0
            groups = [[] for _ in range(max(n_groups, 0))]
            for n, g in enumerate(labels):
                if g >= 0:
                    groups[g].append(n)
            if weights is not None and not isinstance(weights, str):
                node_weights = [float(w) for w in weights]
                if len(node_weights) != self.num_nodes:
                    raise ValueError("with labels=, weights has one entry per node (%d), got %d"
                                     % (self.num_nodes, len(node_weights)))
                weights = [[node_weights[n] for n in g] for g in groups]
        groups = [[int(n) for n in g] for g in groups]
        if len(groups) < 1:
            raise ValueError("a region map needs at least one group")
        for g, members in enumerate(groups):
            for n in members:
                if not 0 <= n < self.num_nodes:
                    raise ValueError("group %d: node index %d outside 0 .. %d" % (g, n, self.num_nodes - 1))
        self.ptr: List[int] = [0]
        self.node: List[int] = []
        for members in groups:
            self.node += members
            self.ptr.append(len(self.node))
        if len(self.node) >= 2 ** 31 or len(groups) >= 2 ** 31:
            raise ValueError("a region map holds fewer than 2^31 groups and members")
        if isinstance(weights, str):
            if weights != "mean":
                raise ValueError("weights=%r: the only named weighting is 'mean'" % (weights,))
            weights = [[1.0 / len(g)] * len(g) if g else [] for g in groups]
        self.weight: Optional[List[float]] = None
        if weights is not None:
            if len(weights) != len(groups):
                raise ValueError("weights has %d lists, expected one per group (%d)" % (len(weights), len(groups)))
            flat: List[float] = []
            for g, (w, members) in enumerate(zip(weights, groups)):
                w = [float(v) for v in w]
                if len(w) != len(members):
                    raise ValueError("group %d: %d weights for %d members" % (g, len(w), len(members)))
                if not all(math.isfinite(v) for v in w):
                    raise ValueError("group %d: weights must be finite" % g)
                flat += w
            # what the device holds: the float32 roundings
            self.weight = torch.tensor(flat, dtype=torch.float32).tolist()
            if not all(math.isfinite(v) for v in self.weight):
                raise ValueError("weights must be finite in float32")
        if names is not None:
            names = [str(v) for v in names]
            if len(names) != len(groups):
                raise ValueError("names has %d entries, expected one per group (%d)" % (len(names), len(groups)))
        self.names: Optional[List[str]] = names
        self._ptr_host = (C.c_int32 * len(self.ptr))(*self.ptr)
        self._device: Dict[torch.device, tuple] = {}
        self._by_node = None                      # the transposed map, derived on first use
        self._node_device: Dict[torch.device, tuple] = {}

    # ---- construction helpers -------------------------------------------------------------------------------------------
    @classmethod
    def singletons(cls, num_nodes: int) -> "RegionMap":
        """one region per node: the totals are the node-level values"""
        return cls(num_nodes, groups=[[n] for n in range(int(num_nodes))])

    @classmethod
    def total(cls, num_nodes: int) -> "RegionMap":
        """one region holding every node"""
        return cls(num_nodes, groups=[list(range(int(num_nodes)))], names=["total"])

    # ---- shape ------------------------------------------------------------------------------------------------------------
    @property
    def num_groups(self) -> int:
        return len(self.ptr) - 1

    @property
    def num_members(self) -> int:
        return len(self.node)

    def members(self, g: int) -> List[int]:
        return self.node[self.ptr[g]:self.ptr[g + 1]]

    def weights_of(self, g: int) -> Optional[List[float]]:
        return None if self.weight is None else self.weight[self.ptr[g]:self.ptr[g + 1]]

    def __len__(self) -> int:
        return self.num_groups

    def __eq__(self, other) -> bool:
        return (isinstance(other, RegionMap) and self.num_nodes == other.num_nodes and self.ptr == other.ptr
                and self.node == other.node and self.weight == other.weight)

    def __ne__(self, other) -> bool:
        return not self.__eq__(other)

    __hash__ = None

    def __repr__(self) -> str:
        return "RegionMap(num_nodes=%d, groups=%d, members=%d, weights=%s)" % (
            self.num_nodes, self.num_groups, self.num_members, "no" if self.weight is None else "yes")

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """plain lists: a map goes into a checkpoint or a JSON file as it is"""
        return {"num_nodes": self.num_nodes, "ptr": list(self.ptr), "node": list(self.node),
                "weight": None if self.weight is None else list(self.weight),
                "names": None if self.names is None else list(self.names)}

    def load_state_dict(self, state: dict) -> "RegionMap":
        self.__init__(**self._init_args(state))
        return self

    @classmethod
    def from_state_dict(cls, state: dict) -> "RegionMap":
        return cls(**cls._init_args(state))

    @staticmethod
    def _init_args(state: dict) -> dict:
        ptr, node, weight = [int(v) for v in state["ptr"]], list(state["node"]), state.get("weight")
        if not ptr or ptr[0] != 0 or ptr[-1] != len(node) or any(b < a for a, b in zip(ptr, ptr[1:])):
            raise ValueError("state_dict: ptr is not a CSR offset list over %d members" % len(node))
        if weight is not None and len(weight) != len(node):
            raise ValueError("state_dict: %d weights for %d members" % (len(weight), len(node)))
        groups = [node[a:b] for a, b in zip(ptr, ptr[1:])]
        weights = None if weight is None else [weight[a:b] for a, b in zip(ptr, ptr[1:])]
        return dict(num_nodes=state["num_nodes"], groups=groups, weights=weights, names=state.get("names"))

    # ---- the device side ----------------------------------------------------------------------------------------------------
    def groups_on(self, device) -> "_lib.Groups":
        """the matgcn_groups descriptor for ``device``; the CSR is uploaded on first use and kept"""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.MatgcnError("a region map is used on the GPU: the hot path is HIP-only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        held = self._device.get(device)
        if held is None:
            ptr = torch.tensor(self.ptr, dtype=torch.int32).to(device)
            node = torch.tensor(self.node, dtype=torch.int32).to(device)
            weight = None if self.weight is None else torch.tensor(self.weight, dtype=torch.float32).to(device)
            held = self._device[device] = (ptr, node, weight)
        ptr, node, weight = held
        g = _lib.Groups()
        g.ptr = C.cast(self._ptr_host, C.POINTER(C.c_int32))
        g.ptr_dev = ptr.data_ptr()
        g.node = node.data_ptr() if self.num_members else None
        g.weight = None if weight is None or not self.num_members else weight.data_ptr()
        g.n_groups, g.n_members = self.num_groups, self.num_members
        return g

    def by_node(self):
        """(ptr, group, weight): the transposed map as plain lists - a CSR list over nodes whose entries are the groups a
        node belongs to, in ascending member position of the by-group map (a stable sort by node), with the weights
        permuted alongside.  Derived, built once; state_dict() does not carry it."""
        held = self._by_node
        if held is None:
            group_of = [g for g in range(self.num_groups) for _ in range(self.ptr[g + 1] - self.ptr[g])]
            order = sorted(range(self.num_members), key=self.node.__getitem__)      # sorted() is stable
            ptr = [0] * (self.num_nodes + 1)
            for n in self.node:
                ptr[n + 1] += 1
            for n in range(self.num_nodes):
                ptr[n + 1] += ptr[n]
            group = [group_of[k] for k in order]
            weight = None if self.weight is None else [self.weight[k] for k in order]
            held = self._by_node = (ptr, group, weight, (C.c_int32 * len(ptr))(*ptr))
        return held[0], held[1], held[2]

    def node_groups_on(self, device) -> "_lib.Groups":
        """the transposed map as a matgcn_groups descriptor for ``device`` (the by_node argument of
        matgcn_region_loss_grad): n_groups = num_nodes, ``node`` holds group indices; uploaded on first use and kept"""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.MatgcnError("a region map is used on the GPU: the hot path is HIP-only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        ptr_l, group_l, weight_l = self.by_node()
        held = self._node_device.get(device)
        if held is None:
            ptr = torch.tensor(ptr_l, dtype=torch.int32).to(device)
            group = torch.tensor(group_l, dtype=torch.int32).to(device)
            weight = None if weight_l is None else torch.tensor(weight_l, dtype=torch.float32).to(device)
            held = self._node_device[device] = (ptr, group, weight)
        ptr, group, weight = held
        g = _lib.Groups()
        g.ptr = C.cast(self._by_node[3], C.POINTER(C.c_int32))
        g.ptr_dev = ptr.data_ptr()
        g.node = group.data_ptr() if self.num_members else None
        g.weight = None if weight is None or not self.num_members else weight.data_ptr()
        g.n_groups, g.n_members = self.num_nodes, self.num_members
        return g
