# NEVER RUN: there is no BEAM where this project is built.  It states, beside the reference's own implementation, what
# tests/test_gpu_mmr_nif.py and tests/test_gpu_mmr_collection.py check through the fake erl_nif runtime and the Python
# mirror: Vettore.Index.FlatGpu.rerank/3 and mmr_search/3 give Vettore.rerank/4's and mmr_rerank/5's answers.
defmodule Vettore.Index.FlatGpuMmrTest do
  use ExUnit.Case, async: false

  alias Vettore.{Collection, Distance, Embedding}
  alias Vettore.Index.FlatGpu

  defp collection(metric, rows) do
    {:ok, collection} = Collection.new(dimensions: length(hd(rows)), metric: metric, index: FlatGpu, normalize: :none)

    embeddings =
      rows |> Enum.with_index() |> Enum.map(fn {v, i} -> %Embedding{id: "doc#{i}", vector: v} end)

    :ok = Collection.put_many(collection, embeddings)
    {collection, Enum.map(embeddings, &{&1.id, &1.vector})}
  end

  defp rows(n, d) do
    :rand.seed(:exsss, {1, 2, 3})
    for _ <- 1..n, do: for(_ <- 1..d, do: :rand.normal())
  end

  test "rerank/3 is Distance.mmr_rerank/5 over the resident rows" do
    for metric <- [:l2, :cosine, :inner_product, :manhattan, :jaccard] do
      {collection, pairs} = collection(metric, rows(60, 8))
      initial = pairs |> Enum.take_random(25) |> Enum.map(fn {id, _} -> {id, :rand.uniform()} end)

      for {alpha, limit} <- [{0.5, 10}, {0.2, 25}, {1, 30}, {0, 1}] do
        assert FlatGpu.rerank(collection, initial, alpha: alpha, limit: limit) ==
                 Distance.mmr_rerank(initial, pairs, metric, alpha, limit)
      end
    end
  end

  test "rerank/3 keeps the reference's doctest, options and errors" do
    {collection, _} = collection(:cosine, [[1.0, 0.0], [0.0, 1.0]])
    assert FlatGpu.rerank(collection, [{"doc0", 0.9}, {"doc1", 0.8}], limit: 1) == {:ok, [{"doc0", 0.9}]}
    assert FlatGpu.rerank(collection, [{"doc0", 0.9}], unknown: true) == {:error, :invalid_options}
    assert FlatGpu.rerank(collection, [{"doc0", 0.9}], alpha: 1.5) == {:error, :invalid_mmr_args}
    assert FlatGpu.rerank(collection, [{"doc0", 0.9}], limit: 0) == {:error, :invalid_mmr_args}
    assert FlatGpu.rerank(collection, [{"nope", 0.9}]) == {:error, :invalid_mmr_args}
    assert FlatGpu.rerank(collection, [{"doc0", 0.9}, {"doc0", 0.1}]) == {:error, :invalid_mmr_args}
    assert FlatGpu.rerank(collection, []) == {:ok, []}
  end

  test "a pair that overflows fails the call in the round that scores it" do
    {collection, _} = collection(:l2_squared, [[0.0], [1.5e19], [-1.5e19]])
    initial = [{"doc0", 3.0}, {"doc1", 2.0}, {"doc2", 1.0}]
    assert FlatGpu.rerank(collection, initial, alpha: 1.0, limit: 2) == {:ok, [{"doc0", 3.0}, {"doc1", 2.0}]}
    assert FlatGpu.rerank(collection, initial, alpha: 1.0, limit: 3) == {:error, :metric_overflow}
  end

  test "mmr_search/3 is search then rerank" do
    for score <- [:raw, :similarity] do
      {:ok, collection} = Collection.new(dimensions: 8, metric: :cosine, index: FlatGpu, score: score)
      :ok = Collection.put_many(collection, rows(200, 8) |> Enum.with_index() |> Enum.map(fn {v, i} -> %Embedding{id: "doc#{i}", vector: v} end))
      query = hd(rows(1, 8))
      {:ok, found} = Collection.search(collection, query, limit: 40)
      {:ok, want} = FlatGpu.rerank(collection, Enum.map(found, &{&1.id, &1.score}), limit: 7, alpha: 0.3)
      {:ok, got} = FlatGpu.mmr_search(collection, query, limit: 7, candidates: 40, alpha: 0.3)
      assert Enum.map(got, &{&1.id, &1.score}) == want
    end
  end
end
