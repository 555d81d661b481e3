defmodule Vettore.Index.HnswGpuTest do
  @moduledoc """
  `Vettore.Index.HnswGpu` beside the reference's own `Vettore.Index.HNSW`: the reference's HNSW is deterministic, so a
  collection built on either answers every search with the same results -- ids, order, scores and distances -- and
  rejects the same options with the same atoms.

  Needs an MI355X (the library has no CPU fallback).  Nobody has run this file: the project's machines have no BEAM.
  What it states is held, on the Python side, by tests/test_gpu_hnsw.py against a restatement of hnsw.rs.
  """
  use ExUnit.Case, async: false

  alias Vettore.Index.{HNSW, HnswGpu}

  defp collection(index, metric, opts) do
    {:ok, c} = Vettore.new(dimensions: 8, metric: metric, normalize: :none, index: index, index_options: opts)
    c
  end

  defp vectors(n) do
    :rand.seed(:exsss, {1, 2, 3})
    for i <- 1..n, do: {"doc-#{rem(i * 7919, 1009)}", for(_ <- 1..8, do: :rand.uniform() * 2 - 1)}
  end

  test "the same results as the reference's HNSW for every supported metric" do
    for metric <- [:l2, :cosine, :inner_product] do
      opts = [m: 4, m0: 8, ef_construction: 40, ef_search: 16]
      gpu = collection(HnswGpu, metric, opts)
      cpu = collection(HNSW, metric, opts)

      for {id, v} <- vectors(300), c <- [gpu, cpu] do
        :ok = Vettore.put(c, %Vettore.Embedding{id: id, vector: v, value: id})
      end

      :ok = Vettore.delete(gpu, "doc-#{rem(7 * 7919, 1009)}")
      :ok = Vettore.delete(cpu, "doc-#{rem(7 * 7919, 1009)}")

      for {_id, q} <- Enum.take(vectors(300), 10), limit <- [1, 10, 400] do
        assert Vettore.search(gpu, q, limit: limit) == Vettore.search(cpu, q, limit: limit), {metric, limit}
      end
    end
  end

  test "an insert gives the rows of deleted nodes back once they outnumber the live ones" do
    gpu = collection(HnswGpu, :cosine, m: 4, m0: 8, ef_construction: 24, ef_search: 12)
    cpu = collection(HNSW, :cosine, m: 4, m0: 8, ef_construction: 24, ef_search: 12)
    docs = vectors(200)

    for {id, v} <- docs, c <- [gpu, cpu] do
      :ok = Vettore.put(c, %Vettore.Embedding{id: id, vector: v, value: id})
    end

    for {id, _v} <- Enum.take(docs, 130), c <- [gpu, cpu] do
      :ok = Vettore.delete(c, id)
    end

    # deletes never compact
    assert {:ok, %{rows: 200, dead_rows: 130, row_capacity: 1024}} = HnswGpu.memory(gpu)

    for c <- [gpu, cpu] do
      :ok = Vettore.put(c, %Vettore.Embedding{id: "one-more", vector: for(_ <- 1..8, do: 0.25), value: "one-more"})
    end

    assert {:ok, %{rows: 71, dead_rows: 0, row_capacity: 1024}} = HnswGpu.memory(gpu)

    for {_id, q} <- Enum.take(docs, 10), limit <- [1, 5, 70] do
      assert Vettore.search(gpu, q, limit: limit) == Vettore.search(cpu, q, limit: limit), limit
    end
  end

  test "quantized, funnel and hybrid searches answer as the reference's composition over the same embeddings" do
    # HnswGpu exports the three functions; the reference composes them from ETS whatever the index is (collection.ex:232-348)
    for metric <- [:l2, :cosine, :inner_product] do
      opts = [m: 4, m0: 8, ef_construction: 40, ef_search: 16]
      gpu = collection(HnswGpu, metric, opts)
      cpu = collection(HNSW, metric, opts)

      for {id, v} <- vectors(300), c <- [gpu, cpu] do
        :ok = Vettore.put(c, %Vettore.Embedding{id: id, vector: v, value: id})
      end

      for {_id, q} <- Enum.take(vectors(300), 5) do
        assert HnswGpu.quantized_search(gpu, q, limit: 7, candidates: 40) == Vettore.quantized_search(cpu, q, limit: 7, candidates: 40)
        assert HnswGpu.funnel_search(gpu, q, limit: 7, stages: [3, 6]) == Vettore.funnel_search(cpu, q, limit: 7, stages: [3, 6])
        assert HnswGpu.hybrid_search(gpu, q, limit: 7) == Vettore.hybrid_search(cpu, q, limit: 7)
        assert HnswGpu.hybrid_search(gpu, q, generators: [:hnsw, {:funnel, stages: [4]}]) ==
                 Vettore.hybrid_search(cpu, q, generators: [:hnsw, {:funnel, stages: [4]}])
      end

      assert HnswGpu.funnel_search(gpu, for(_ <- 1..8, do: 0.5), stages: [9]) == {:error, :invalid_stages}
      assert HnswGpu.quantized_search(gpu, for(_ <- 1..8, do: 0.5), limit: 0) == {:error, :invalid_limit}
    end
  end

  test "options and metrics are rejected as hnsw.ex rejects them" do
    for bad <- [[m: 0], [m0: 2_049], [m: 16, m0: 8], [ef_construction: 8], [ef_search: 0], [max_level: 65], [unknown: 1], [m: 8, m: 8], :m] do
      assert HnswGpu.new(:l2, bad) == {:error, :invalid_hnsw_options}
      if is_list(bad) and not Keyword.has_key?(bad, :unknown), do: assert(HNSW.new(:l2, bad) == {:error, :invalid_hnsw_options})
    end

    assert HnswGpu.new(:hamming, []) == {:error, {:unsupported_hnsw_metric, :hamming}}
    assert HnswGpu.defaults() == HNSW.defaults()
  end
end
