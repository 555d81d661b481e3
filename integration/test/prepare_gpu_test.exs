# NEVER RUN: there is no BEAM where this project is built.  It states, beside the reference's own implementation, what
# tests/test_gpu_prepare_nif.py and tests/test_gpu_prepare_collection.py check through the fake erl_nif runtime and the
# Python mirror: the device's normalize_zscore/1, normalize_minmax/1 and prepare_rows/2 give Vettore.Nifs' and
# Collection.prepare_embedding's answers.
defmodule Vettore.Index.FlatGpuPrepareTest do
  use ExUnit.Case, async: false

  alias Vettore.{Collection, Embedding, Nifs}
  alias Vettore.Index.FlatGpu

  defp rows(n, d) do
    :rand.seed(:exsss, {14, 14, 14})
    constant = List.duplicate(4.0, d)
    zeros = List.duplicate(0.0, d)
    [constant, zeros | for(_ <- 1..n, do: for(_ <- 1..d, do: :rand.normal() * 100.0))]
  end

  test "normalize_zscore/1 and normalize_minmax/1 are the reference NIFs'" do
    for vector <- rows(20, 70) ++ [[], [5.0]] do
      assert FlatGpu.normalize_zscore(vector) == Nifs.normalize_zscore(vector)
      assert FlatGpu.normalize_minmax(vector) == Nifs.normalize_minmax(vector)
    end

    # distances.rs:525-526, :664-665; vector_distance_test.exs:93-102
    assert FlatGpu.normalize_zscore([4.0, 4.0]) == {:ok, [0.0, 0.0]}
    assert FlatGpu.normalize_minmax([7.0, 7.0]) == {:ok, [0.0, 0.0]}
    assert FlatGpu.normalize_minmax([-7.0, 0.0, 21.0]) == {:ok, [0.0, 0.25, 1.0]}
    assert FlatGpu.normalize_minmax([2.0, 4.0, 6.0]) == {:ok, [0.0, 0.5, 1.0]}
  end

  test "prepare_rows/2 is normalize + compress_sign_bits per vector" do
    vectors = rows(130, 70)

    for {mode, normalize} <- [
          none: &{:ok, &1},
          l2: &Nifs.normalize_l2/1,
          zscore: &Nifs.normalize_zscore/1,
          minmax: &Nifs.normalize_minmax/1
        ] do
      expected =
        Enum.map(vectors, fn v ->
          {:ok, normalized} = normalize.(v)
          {normalized, Nifs.compress_sign_bits(normalized)}
        end)

      assert FlatGpu.prepare_rows(mode, vectors) == {:ok, expected}
    end

    assert FlatGpu.prepare_rows(:l2, []) == {:ok, []}
    assert_raise ArgumentError, fn -> FlatGpu.prepare_rows(:l1, vectors) end
    assert_raise ArgumentError, fn -> FlatGpu.prepare_rows(:l2, [[1.0, 2.0], [1.0]]) end
  end

  test "a collection with normalize: :zscore or :minmax opens on the GPU index and stores the reference's rows" do
    vectors = rows(50, 16)

    for normalize <- [:none, :l2, :zscore, :minmax] do
      {:ok, gpu} = Collection.new(dimensions: 16, metric: :cosine, index: FlatGpu, normalize: normalize)
      {:ok, cpu} = Collection.new(dimensions: 16, metric: :cosine, normalize: normalize)
      embeddings = vectors |> Enum.with_index() |> Enum.map(fn {v, i} -> %Embedding{id: "doc#{i}", vector: v} end)
      :ok = Collection.put_many(gpu, embeddings)
      :ok = Collection.put_many(cpu, embeddings)
      {:ok, from_gpu} = Collection.all(gpu)
      {:ok, from_cpu} = Collection.all(cpu)
      assert Enum.sort_by(from_gpu, & &1.id) == Enum.sort_by(from_cpu, & &1.id)
      query = hd(Enum.drop(vectors, 5))
      assert Collection.prepare_query(gpu, query) == Collection.prepare_query(cpu, query)
    end
  end
end
