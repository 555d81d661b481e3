defmodule Vettore.Index.HnswGpu do
  @moduledoc """
  `Vettore.Index` implementation (lib/vettore/index.ex:12-17) of the reference's HNSW index on an MI355X.

      Vettore.new(dimensions: 768, metric: :cosine, index: Vettore.Index.HnswGpu,
                  index_options: [m: 16, m0: 32, ef_construction: 100, ef_search: 64, device: 0])

  Same steps and the same errors as `Vettore.Index.HNSW` (lib/vettore/index/hnsw.ex): options are normalised and
  checked before the metric, `search/3` prepares the query itself and drops hits whose id is no longer in ETS.  The
  graph is the reference's node for node -- levels from the id's hash, neighbour selection by (distance, internal
  id) -- and so are the hits: ids, order (rank, then id bytes) and raw values.  `device:` is the one extra option.
  """
  @behaviour Vettore.Index

  alias Vettore.{Collection, Distance, Embedding, Result}
  alias Vettore.Gpu.Nifs
  alias Vettore.Index.FlatGpu

  @default_options [m: 16, m0: 32, ef_construction: 100, ef_search: 64, max_level: 12]
  @option_keys Keyword.keys(@default_options)
  @max_m 1_024
  @max_m0 2_048
  @max_ef 1_000_000
  @max_level 64
  @max_nif_usize 4_294_967_295

  @impl true
  def new(metric, opts \\ []) do
    with {:ok, options, device} <- normalize_options(opts) do
      new_metric(metric, options, device)
    end
  end

  def defaults, do: @default_options

  @impl true
  def put(%Collection{index_state: ref}, %Embedding{id: id, vector: vector}),
    do: unit(Nifs.hnsw_insert(ref, id, vector))

  @impl true
  def put_many(%Collection{index_state: ref}, embeddings),
    do: unit(Nifs.hnsw_insert_many(ref, Enum.map(embeddings, &{&1.id, &1.vector})))

  @impl true
  def delete(%Collection{index_state: ref}, id), do: unit(Nifs.hnsw_delete(ref, id))

  @impl true
  def search(%Collection{} = collection, query, opts) do
    with :ok <- validate_search_options(opts),
         limit = Keyword.get(opts, :limit, 10),
         :ok <- validate_limit(limit),
         {:ok, query} <- Collection.prepare_query(collection, query),
         {:ok, hits} <- Nifs.hnsw_search(collection.index_state, query, limit) do
      {:ok, Enum.flat_map(hits, &to_result(collection, &1))}
    end
  end

  # ---- the collection's staged searches on the index's own rows ---------------------------------
  # With the dispatch of INTEGRATION.md section 3 in collection.ex (`function_exported?(collection.index_mod, ...)`)
  # `Vettore.quantized_search/3`, `funnel_search/3` and `hybrid_search/3` land here instead of the reference's ETS
  # composition, with identical answers: the slab holds the vectors as given and the stages order by (rank, id).  The
  # option handling is Vettore.Index.FlatGpu's; `:hnsw` and `:search` are both the index's own traversal, and
  # hybrid_search defaults to `[:hnsw, :quantized]` (collection.ex:513).

  @doc "collection.ex:276-295 on the index's rows."
  def quantized_search(%Collection{} = collection, query, opts \\ []) do
    with {:ok, limit, candidates} <- FlatGpu.staged_limit_and_candidates(opts),
         {:ok, prepared} <- Collection.prepare_query(collection, query),
         {:ok, hits} <- Nifs.hnsw_quantized_search(collection.index_state, prepared, candidates, limit) do
      {:ok, Enum.flat_map(hits, &to_result(collection, &1))}
    end
  end

  @doc "collection.ex:245-260 on the index's rows."
  def funnel_search(%Collection{dimensions: d} = collection, query, opts \\ []) do
    with {:ok, limit, candidates} <- FlatGpu.staged_limit_and_candidates(opts),
         {:ok, stages} <- FlatGpu.staged_stages(d, opts),
         {:ok, prepared} <- Collection.prepare_query(collection, query),
         {:ok, hits} <- Nifs.hnsw_funnel_search(collection.index_state, prepared, stages, candidates, limit) do
      {:ok, Enum.flat_map(hits, &to_result(collection, &1))}
    end
  end

  @doc "collection.ex:325-345 with `rerank: :exact` on the index's rows; the default generators are `[:hnsw, :quantized]`."
  def hybrid_search(%Collection{dimensions: d} = collection, query, opts \\ []) do
    limit = Keyword.get(opts, :limit, 10)
    generators = Keyword.get(opts, :generators, [:hnsw, :quantized])
    rerank = Keyword.get(opts, :rerank, :exact)

    with :ok <- FlatGpu.staged_limit(limit),
         {:ok, prepared} <- Collection.prepare_query(collection, query),
         {:ok, spec} <- FlatGpu.staged_generators(generators, d, limit, true),
         :ok <- if(rerank == :exact, do: :ok, else: {:error, {:invalid_rerank, rerank}}),
         {:ok, hits} <- Nifs.hnsw_hybrid_search(collection.index_state, prepared, spec, limit) do
      {:ok, Enum.flat_map(hits, &to_result(collection, &1))}
    end
  end

  @doc """
  What the index holds on the device: `{:ok, %{rows: _, row_capacity: _, dead_rows: _, edges: _}}`.  `rows` are the slab
  rows handed out since the last compaction and `dead_rows` those of them whose node was deleted or replaced.  An insert
  that finds more dead rows than live ones, and at least 64 of them, compacts first: `dead_rows` is 0 again, `rows` the
  live count, and `row_capacity` may shrink.  A delete never compacts.
  """
  def memory(%Collection{index_state: ref}) do
    with {:ok, {rows, row_capacity, dead_rows, edges}} <- Nifs.hnsw_memory(ref) do
      {:ok, %{rows: rows, row_capacity: row_capacity, dead_rows: dead_rows, edges: edges}}
    end
  end

  defp to_result(collection, {id, raw}) do
    case Collection.get(collection, id) do
      {:ok, %Embedding{} = embedding} ->
        {score, distance} = Distance.result_values(collection.metric, raw, collection.score)

        [
          %Result{
            id: id,
            value: embedding.value,
            score: score,
            distance: distance,
            metric: collection.metric,
            metadata: embedding.metadata
          }
        ]

      {:error, _reason} ->
        []
    end
  end

  defp unit({:ok, {}}), do: :ok
  defp unit(:ok), do: :ok
  defp unit(other), do: other

  defp validate_limit(limit) when is_integer(limit) and limit > 0 and limit <= @max_nif_usize, do: :ok
  defp validate_limit(_limit), do: {:error, :invalid_limit}

  defp validate_search_options(opts) when is_list(opts) do
    if Keyword.keyword?(opts) and Enum.all?(Keyword.keys(opts), &(&1 == :limit)),
      do: :ok,
      else: {:error, :invalid_search_options}
  end

  defp validate_search_options(_opts), do: {:error, :invalid_search_options}

  defp new_metric(:l2, o, device), do: apply_new(&Nifs.hnsw_new_l2/6, o, device)
  defp new_metric(:cosine, o, device), do: apply_new(&Nifs.hnsw_new_cosine/6, o, device)
  defp new_metric(:inner_product, o, device), do: apply_new(&Nifs.hnsw_new_inner_product/6, o, device)
  defp new_metric(metric, _o, _device), do: {:error, {:unsupported_hnsw_metric, metric}}

  defp apply_new(fun, o, device),
    do: fun.(o[:m], o[:m0], o[:ef_construction], o[:ef_search], o[:max_level], device)

  defp normalize_options(opts) when is_list(opts) do
    with true <- Keyword.keyword?(opts),
         true <- Enum.all?(Keyword.keys(opts), &(&1 in [:device | @option_keys])),
         true <- length(Keyword.keys(opts)) == MapSet.size(MapSet.new(Keyword.keys(opts))),
         {device, opts} = Keyword.pop(opts, :device, 0),
         true <- is_integer(device) and device >= 0,
         options = Keyword.merge(@default_options, opts),
         true <- valid_options?(options) do
      {:ok, options, device}
    else
      _ -> {:error, :invalid_hnsw_options}
    end
  end

  defp normalize_options(_opts), do: {:error, :invalid_hnsw_options}

  defp pos?(value), do: is_integer(value) and value > 0

  defp valid_options?(o) do
    pos?(o[:m]) and o[:m] <= @max_m and pos?(o[:m0]) and o[:m0] >= o[:m] and o[:m0] <= @max_m0 and
      pos?(o[:ef_construction]) and o[:ef_construction] >= o[:m] and o[:ef_construction] <= @max_ef and
      pos?(o[:ef_search]) and o[:ef_search] <= @max_ef and pos?(o[:max_level]) and o[:max_level] <= @max_level
  end
end
