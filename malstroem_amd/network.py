"""Stream network and rain events -- mirror of ``malstroem.network`` (reference network.py:20-129).

Same class, same node dictionaries (``nodeid``, ``dstrnodeid``, ``wshed_area``, ``bspot_vol``), same results in the same
order; the leaf-to-root fill / spill pass runs in the library for ALL requested events at once (``mhip_rain_events``)
instead of one Python recursion per event.
"""
import ctypes
from collections import defaultdict

import numpy as np

from . import _lib


class Network(object):
    """Stream network: ``nodes``, ``root_nodes`` (no downstream node), ``upstream_tree`` (node id -> ids one step upstream)."""

    def __init__(self):
        self.nodes = []
        self.nodes_index = {}
        self.root_nodes = []
        self.upstream_tree = defaultdict(list)

    def add_nodes(self, nodes):
        for n in nodes:
            self.add_node(n)

    def add_node(self, node):
        self.nodes.append(node)
        node_id, downstream_id = node['nodeid'], node['dstrnodeid']
        self.nodes_index[node_id] = node
        self.upstream_tree[downstream_id].append(node_id)
        if downstream_id is None:
            self.root_nodes.append(node_id)

    def rain_events(self, events_mm, area_key="wshed_area"):
        """Every event of ``events_mm`` in one pass -> list (per event) of lists of event dicts
        ``{nodeid, rainv, spillv, v, pctv}`` in the reference's order (network.py:115-129).  ``area_key``: the node property that
        is the area the rain falls on -- ``wshed_eff_area`` for the runoff-weighted area of ``runoff.py``; the default is the
        reference's."""
        events = np.ascontiguousarray(np.asarray(list(events_mm), dtype=np.float64))
        n = len(self.nodes)
        # the LAST node added under an id is the one the reference evaluates (nodes_index keeps the last), but every add
        # contributes an upstream entry; ids are unique in practice
        pos = {node['nodeid']: i for i, node in enumerate(self.nodes)}
        down = np.empty(n, dtype=np.int64)
        for i, node in enumerate(self.nodes):
            d = node['dstrnodeid']
            down[i] = -1 if d is None else pos.get(d, -2)
        area = np.array([float(node[area_key]) for node in self.nodes], dtype=np.float64)
        vol = np.array([float(node['bspot_vol']) for node in self.nodes], dtype=np.float64)
        ne = len(events)
        out = [np.zeros((ne, n), dtype=np.float64) for _ in range(4)]
        order = np.zeros(max(n, 1), dtype=np.int64)
        ncomp = ctypes.c_int64(0)
        _lib.call("mhip_rain_events", _lib.i64(n), _lib.ptr(down), _lib.ptr(area), _lib.ptr(vol), ctypes.c_int32(ne), _lib.ptr(events),
                  _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(out[3]), _lib.ptr(order), ctypes.byref(ncomp))
        rainv, spillv, v, pctv = out
        results = []
        for e in range(ne):
            ev = []
            for i in order[:ncomp.value].tolist():
                p = pctv[e, i]
                ev.append(dict(nodeid=self.nodes[i]['nodeid'], rainv=float(rainv[e, i]), spillv=float(spillv[e, i]) if spillv[e, i] else 0,
                               v=float(v[e, i]), pctv=None if p != p else float(p)))
            results.append(ev)
        return results

    def rain_event(self, mmrain, area_key="wshed_area"):
        """All nodes below a root with the event's values added (network.py:115-129)."""
        return self.rain_events([mmrain], area_key)[0]
