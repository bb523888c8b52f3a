"""The decoder of the splat's state block (``_lib.SplatState``) against the rule written out here.  CPU only: no library call."""
import itertools

import pytest
import torch

from gaussianformer_amd import _lib

PATHS = {"GF_PATH_EXACT_TILE": 0, "GF_PATH_MATRIX_CORE": 1, "GF_PATH_ARBITRARY": 2, "GF_PATH_MATRIX_CORE_WAVE": 3,
         "GF_PATH_MATRIX_CORE_PAIR": 4, "GF_PATH_MATRIX_CORE_SOLO": 5}


def test_the_path_names_and_the_matrix_core_set():
    assert {n: getattr(_lib, n) for n in dir(_lib) if n.startswith("GF_PATH_")} == PATHS
    four = ("GF_PATH_MATRIX_CORE", "GF_PATH_MATRIX_CORE_WAVE", "GF_PATH_MATRIX_CORE_PAIR", "GF_PATH_MATRIX_CORE_SOLO")
    assert sorted(_lib.GF_PATHS_MATRIX_CORE) == sorted(PATHS[n] for n in four) and len(_lib.GF_PATHS_MATRIX_CORE) == 4


@pytest.mark.parametrize("path,word0,word4", itertools.product(sorted(PATHS.values()), (0, 1), (0, 1, 2)))
def test_decoder_against_the_rule(path, word0, word4):
    """Word 0 != 0: not dense; word 1: the path; word 2: verdict bits; word 3: generation; word 4: bit 0 ready, bit 1 overflow;
    on matrix cores = word 0 is 0 and word 1 is 1, 3, 4 or 5."""
    verdict, generation = (path * 5 + word4) % 16, -7 - path   # (an int32 view shows a generation past 2^31 as negative)
    st = _lib.SplatState.of([word0, path, verdict, generation, word4])
    assert st == (word0 == 1, path, verdict, generation, word4 == 1, word4 == 2, word0 == 0 and path in (1, 3, 4, 5))
    assert (st.not_dense, st.path, st.verdict, st.generation, st.rows_ready, st.rows_overflow, st.on_matrix_cores) == tuple(st)


def test_tensor_form_and_short_lists():
    """A state tensor -- the uint8 block or an int32 view -- decodes like its words; words a caller did not read count as 0."""
    words = [0, _lib.GF_PATH_MATRIX_CORE_WAVE, _lib.GF_VERDICT_THETA | _lib.GF_VERDICT_OPASEM, 12345, _lib.GF_ROWS_READY | _lib.GF_ROWS_OVERFLOW]
    want = _lib.SplatState.of(words)
    assert want == (False, 3, 12, 12345, True, True, True) and _lib.STATE_USED_BYTES == 4 * _lib.GF_STATE_WORDS == 20
    block = torch.full((256,), 255, dtype=torch.uint8)   # (what lies past the words is not read)
    block[:20].view(torch.int32).copy_(torch.tensor(words, dtype=torch.int32))
    assert _lib.SplatState.of(block) == want and _lib.SplatState.of(block.view(torch.int32)) == want
    assert _lib.SplatState.of(words[:3]) == (False, 3, 12, 0, False, False, True)
