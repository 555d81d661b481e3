"""A resident multi-vector store: documents -- lists of vectors -- put once and kept in device memory, searched by
MaxSim (K9r; K9rb for many query sets in one call) without another upload.  A thin object over the vt_mv_* entry points (include/vettore_flat.h): a search
returns what `nifs.multi_vector_top_k` returns for the live documents in the order of their last put, bit for bit."""
from __future__ import annotations

from . import nifs


class ResidentMultiVector:
    def __init__(self, device=None):
        self.ref = nifs.mv_new(device)

    def put_many(self, documents):
        """Upsert [(id, [[float]])]; all or nothing: "ok" or ("error", reason)."""
        return nifs.mv_put_many(self.ref, documents)

    def delete(self, id_):
        """An unknown id is "ok" as well."""
        return nifs.mv_delete(self.ref, id_)

    def top_k(self, query_vectors, metric_code, limit):
        return nifs.mv_top_k(self.ref, query_vectors, metric_code, limit)

    def top_k_ids(self, ids, query_vectors, metric_code, limit):
        """Over the listed live documents only: unknown ids are skipped, a duplicate counts once."""
        return nifs.mv_top_k_ids(self.ref, ids, query_vectors, metric_code, limit)

    def top_k_batch(self, query_sets, metric_code, limit):
        """top_k for every query set in one call: [("ok", hits) | ("error", reason)], each what top_k returns for that
        set alone on the same store state; ("error", reason) when the call itself fails."""
        return nifs.mv_top_k_batch(self.ref, query_sets, metric_code, limit)

    def top_k_ids_batch(self, id_lists, query_sets, metric_code, limit):
        """top_k_ids for every (id list, query set) pair in one call."""
        return nifs.mv_top_k_ids_batch(self.ref, id_lists, query_sets, metric_code, limit)

    # MUVERA retrieval: `config` is (dimension, num_repetitions, num_simhash_projections, seed, projection_dimension,
    # final_projection_dimension | None); `index` a single-shard inner-product FlatRef on the store's device
    def encode_documents(self, ids, config):
        """The listed documents' document-mode encodings, computed from the resident rows (K10s)."""
        return nifs.mv_encode_documents(self.ref, ids, config)

    def fde_sync(self, index, ids, config):
        """Brings `index` in line with the store for `ids` (None: every live document)."""
        return nifs.mv_fde_sync(self.ref, index, ids, config)

    def fde_top_k(self, index, config, query_vectors, candidates, metric_code, limit):
        """Candidates from `index` by the query's encoding, reranked with exact MaxSim."""
        return nifs.mv_fde_top_k(self.ref, index, config, query_vectors, candidates, metric_code, limit)

    def fde_top_k_batch(self, index, config, query_sets, candidates, metric_code, limit):
        return nifs.mv_fde_top_k_batch(self.ref, index, config, query_sets, candidates, metric_code, limit)

    def counters(self):
        """{"scoring_launches", "batched_sets"}: MaxSim kernel launches and query sets scored by K9rb since the store was made."""
        return nifs.mv_counters(self.ref)

    def memory(self):
        return nifs.mv_memory(self.ref)

    def __len__(self):
        return nifs.mv_len(self.ref)

    @property
    def dimension(self):
        return nifs.mv_dimension(self.ref)
