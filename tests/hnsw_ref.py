"""The reference's HNSW index (native/vettore/src/hnsw.rs) restated function by function, the reference way: real
heaps, a prune that recomputes every distance and sorts, hash maps keyed by internal ids that are never reused.
Distances come from the CPU oracle (oracle.compute / oracle.rank_value), so a test can hold the device to the graph
and to the hits bit for bit.  The lane order of every 8-float chunk is the oracle's (oracle.set_reduce_order): set it
to the library's first.  Errors carry the reference's strings."""
import heapq
import struct

import numpy as np

import oracle

L2, COSINE, INNER_PRODUCT = 0, 2, 3


class HnswError(Exception):
    """Carries the reference's error string."""


def validate_params(m, m0, ef_construction, ef_search, max_level):  # hnsw.rs:25-49
    if m == 0:
        raise HnswError("m must be positive")
    if m0 == 0:
        raise HnswError("m0 must be positive")
    if m > 1024 or m0 > 2048 or m0 < m:
        raise HnswError("invalid hnsw degree")
    if ef_construction < m:
        raise HnswError("ef_construction must be >= m")
    if ef_construction > 1_000_000:
        raise HnswError("ef_construction exceeds safety limit")
    if ef_search == 0 or ef_search > 1_000_000:
        raise HnswError("ef_search must be positive")
    if max_level == 0 or max_level > 64:
        raise HnswError("max_level must be positive")


def total_key(dist):
    """f32::total_cmp as an order-preserving integer."""
    u = struct.unpack("<I", struct.pack("<f", dist))[0]
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def hash64(data: bytes) -> int:  # hnsw.rs:490-497
    h = 0xCBF29CE484222325
    for byte in data:
        h ^= byte
        h = (h * 0x00000100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def validate_vector(vector, dimension):  # hnsw.rs:499-507
    if len(vector) == 0:
        raise HnswError("vector must not be empty")
    if dimension is not None and len(vector) != dimension:
        raise HnswError("dimension mismatch")
    if not np.all(np.isfinite(vector)):
        raise HnswError("vector contains a non-finite value")


class Node:
    def __init__(self, external_id, vector, connections, layer):
        self.external_id, self.vector, self.connections, self.layer = external_id, vector, connections, layer


class HnswIndex:
    def __init__(self, metric, m=16, m0=32, ef_construction=100, ef_search=64, max_level=12):
        validate_params(m, m0, ef_construction, ef_search, max_level)
        self.metric = metric
        self.m, self.m0, self.ef_construction, self.ef_search, self.max_level = m, m0, ef_construction, ef_search, max_level
        self.nodes = {}
        self.external_to_internal = {}
        self.entry = None
        self.next = 0
        self.dimension = None
        self.distance_calls = 0
        # what the last insert's search_layer calls returned, {layer: [(internal id, dist)]} in heap order
        self.last_lists = {}

    def __len__(self):
        return len(self.nodes)

    # hnsw.rs:468-470
    def rank_distance(self, left, right):
        self.distance_calls += 1
        try:
            raw = oracle.compute(self.metric, left, right)
        except oracle.OracleError as e:
            raise HnswError(str(e))
        return float(oracle.rank_value(self.metric, raw))

    def level_for(self, external_id: bytes):  # hnsw.rs:473-481
        h = hash64(external_id)
        level = 0
        while level < self.max_level and h & 3 == 0:
            level += 1
            h >>= 2
        return level

    def insert(self, external_id, vector):  # hnsw.rs:152-245
        external_id = external_id.encode() if isinstance(external_id, str) else bytes(external_id)
        vector = np.ascontiguousarray(np.asarray(vector, dtype=np.float32).reshape(-1))
        validate_vector(vector, self.dimension)
        if external_id in self.external_to_internal:
            self.delete(external_id)
        internal_id = self.next
        self.next += 1
        node_level = self.level_for(external_id)
        self.last_lists = {}
        if not self.nodes:
            self.nodes[internal_id] = Node(external_id, vector, [[] for _ in range(node_level + 1)], node_level)
            self.external_to_internal[external_id] = internal_id
            self.entry = internal_id
            self.dimension = len(vector)
            return
        entry = self.entry
        top_layer = self.nodes[entry].layer
        for layer in range(top_layer, node_level, -1):
            entry, _ = self.greedy_closest(entry, vector, layer)
        new_connections = [[] for _ in range(node_level + 1)]
        for layer in range(min(node_level, top_layer), -1, -1):
            candidates = self.search_layer(entry, vector, layer, self.ef_construction)
            self.last_lists[layer] = list(candidates)
            candidates.sort(key=lambda c: (total_key(c[1]), c[0]))
            dedup = []
            for c in candidates:
                if not dedup or dedup[-1][0] != c[0]:
                    dedup.append(c)
            candidates = dedup[:self.m0 if layer == 0 else self.m]
            new_connections[layer] = [c[0] for c in candidates]
            if candidates:
                entry = candidates[0][0]
        self.nodes[internal_id] = Node(external_id, vector, new_connections, node_level)
        self.external_to_internal[external_id] = internal_id
        self.dimension = len(vector)
        for layer, neighbors in enumerate([list(c) for c in new_connections]):
            for neighbor_id in neighbors:
                node = self.nodes.get(neighbor_id)
                if node is not None and layer < len(node.connections) and internal_id not in node.connections[layer]:
                    node.connections[layer].append(internal_id)
                self.prune(neighbor_id, layer)
        if self.entry is not None and node_level > self.nodes[self.entry].layer:
            self.entry = internal_id

    def insert_many(self, vectors):  # hnsw.rs:249-260
        vectors = [(i, np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))) for i, v in vectors]
        expected = self.dimension if self.dimension is not None else (len(vectors[0][1]) if vectors else None)
        for _, v in vectors:
            validate_vector(v, expected)
        for i, v in vectors:
            self.insert(i, v)

    def delete(self, external_id):  # hnsw.rs:263-289
        external_id = external_id.encode() if isinstance(external_id, str) else bytes(external_id)
        internal_id = self.external_to_internal.pop(external_id, None)
        if internal_id is None:
            return
        del self.nodes[internal_id]
        for node in self.nodes.values():
            node.connections = [[i for i in layer if i != internal_id] for layer in node.connections]
        if self.entry == internal_id:
            self.entry = None
            best = None
            for nid, node in self.nodes.items():  # max by (layer, reversed external id)
                if best is None or node.layer > best.layer or (node.layer == best.layer and node.external_id < best.external_id):
                    best, self.entry = node, nid
        if not self.nodes:
            self.dimension = None

    def search(self, query, limit):  # hnsw.rs:292-333
        if limit == 0:
            return []
        query = np.ascontiguousarray(np.asarray(query, dtype=np.float32).reshape(-1))
        validate_vector(query, self.dimension)
        if self.entry is None:
            return []
        entry = self.entry
        for layer in range(self.nodes[entry].layer, 0, -1):
            entry = self.greedy_closest(entry, query, layer)[0]
        best = self.search_layer(entry, query, 0, max(self.ef_search, limit))
        best.sort(key=lambda c: (total_key(c[1]), self.nodes[c[0]].external_id))
        out = []
        for nid, _ in best[:limit]:
            node = self.nodes[nid]
            try:
                raw = oracle.compute(self.metric, query, node.vector)
            except oracle.OracleError as e:
                raise HnswError(str(e))
            out.append((node.external_id, np.float32(raw)))
        return out

    def greedy_closest(self, start, query, layer):  # hnsw.rs:336-372
        current = start
        current_dist = self.rank_distance(self.nodes[current].vector, query)
        while True:
            moved = False
            node = self.nodes.get(current)
            if node is None or layer >= len(node.connections):
                break
            for neighbor_id in node.connections[layer]:
                neighbor = self.nodes.get(neighbor_id)
                if neighbor is None:
                    continue
                dist = self.rank_distance(neighbor.vector, query)
                if dist < current_dist:
                    current, current_dist, moved = neighbor_id, dist, True
            if not moved:
                break
        return current, current_dist

    def search_layer(self, entry, query, layer, ef):  # hnsw.rs:375-434
        if entry not in self.nodes:
            return []
        visited = set()
        candidates, results = [], []  # (key, id, dist) min-heap; (-key, -id, dist) max-heap
        dist = self.rank_distance(self.nodes[entry].vector, query)
        heapq.heappush(candidates, (total_key(dist), entry, dist))
        heapq.heappush(results, (-total_key(dist), -entry, dist))
        visited.add(entry)
        while candidates:
            _, cur_id, cur_dist = heapq.heappop(candidates)
            worst = results[0][2] if results else float("inf")
            if len(results) >= ef and cur_dist > worst:
                break
            node = self.nodes.get(cur_id)
            if node is None or layer >= len(node.connections):
                continue
            for neighbor_id in node.connections[layer]:
                if neighbor_id in visited:
                    continue
                visited.add(neighbor_id)
                neighbor = self.nodes.get(neighbor_id)
                if neighbor is None:
                    continue
                dist = self.rank_distance(neighbor.vector, query)
                if len(results) < ef or dist < worst:
                    heapq.heappush(candidates, (total_key(dist), neighbor_id, dist))
                    heapq.heappush(results, (-total_key(dist), -neighbor_id, dist))
                    if len(results) > ef:
                        heapq.heappop(results)
        return [(-nid, dist) for _, nid, dist in results]

    def prune(self, node_id, layer):  # hnsw.rs:437-465
        limit = self.m0 if layer == 0 else self.m
        node = self.nodes.get(node_id)
        if node is None or layer >= len(node.connections):
            return
        scored = []
        for neighbor_id in node.connections[layer]:
            neighbor = self.nodes.get(neighbor_id)
            if neighbor is not None:
                scored.append((neighbor_id, self.rank_distance(node.vector, neighbor.vector)))
        scored.sort(key=lambda s: (total_key(s[1]), s[0]))
        node.connections[layer] = [s[0] for s in scored[:limit]]
