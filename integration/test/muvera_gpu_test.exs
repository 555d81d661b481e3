defmodule Vettore.Index.FlatGpuMuveraTest do
  @moduledoc """
  `muvera_encode_query/7` and `muvera_encode_document/7` of `Vettore.Index.FlatGpu` beside the reference's own
  NIFs: `tests/golden/muvera_rs.json` holds the reference's known answers as data (each with its `cite`), and
  every case here goes through both -- the GPU's encoding must be the reference's list, float for float, and
  its error the reference's string.

  Needs an MI355X (the library has no CPU fallback).
  """
  use ExUnit.Case, async: false

  alias Vettore.Index.FlatGpu

  @fixture Path.expand("../../tests/golden/muvera_rs.json", __DIR__)
  @golden @fixture |> File.read!() |> JSON.decode!()

  defp args(vectors, c) do
    [
      vectors,
      c["dimension"],
      c["num_repetitions"],
      c["num_simhash_projections"],
      c["seed"],
      c["projection_dimension"],
      c["final_projection_dimension"]
    ]
  end

  defp encode(module, "query", a), do: apply(module, :muvera_encode_query, a)
  defp encode(module, "document", a), do: apply(module, :muvera_encode_document, a)

  test "every golden case without a NaN agrees with the reference's NIF" do
    for c <- @golden["cases"], not Enum.any?(List.flatten(c["vectors"]), &is_binary/1) do
      a = args(c["vectors"], c["config"])
      assert encode(FlatGpu, c["mode"], a) == encode(Vettore.Nifs, c["mode"], a), c["name"]

      case c["expect"] do
        %{"ok" => want} -> assert {:ok, got} = encode(FlatGpu, c["mode"], a)
                           assert length(got) == length(want)
        %{"len" => n} -> assert {:ok, got} = encode(FlatGpu, c["mode"], a)
                         assert length(got) == n
        %{"string" => s} -> assert {:error, ^s} = encode(FlatGpu, c["mode"], a)
        %{"error" => s} -> assert {:error, ^s} = encode(FlatGpu, c["mode"], a)
      end
    end
  end

  test "nil and an integer are told apart, and the seed is a full u64" do
    v = [[1.0, 0.0], [0.0, 1.0]]
    assert {:ok, [1.0, 1.0]} = FlatGpu.muvera_encode_query(v, 2, 1, 0, 42, 2, nil)
    assert {:error, "final_projection_dimension must be positive"} = FlatGpu.muvera_encode_query(v, 2, 1, 0, 42, 2, 0)
    assert {:ok, five} = FlatGpu.muvera_encode_query(v, 2, 2, 1, 18_446_744_073_709_551_615, 3, 5)
    assert five == elem(Vettore.Nifs.muvera_encode_query(v, 2, 2, 1, 18_446_744_073_709_551_615, 3, 5), 1)
    assert_raise ArgumentError, fn -> FlatGpu.muvera_encode_query(v, 2, 1, 0, 42, 2, :none) end
    assert_raise ArgumentError, fn -> FlatGpu.muvera_encode_query(v, 2, 1, 0, -1, 2, nil) end
  end
end
