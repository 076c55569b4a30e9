"""lcpc_proof_of_storage_amd -- MI355X-native lcpc-2d commit/prove/verify row-encoding path.

Drop-in for the reference's LcEncoding / LcCommit / LcEvalProof path
(TrevorGKann/lcpc_proof_of_storage, lcpc-2d + lcpc-ligero-pc) behind the C ABI in
include/lcpc_mi.h, implemented by liblcpc_mi.so (gfx950 HIP kernels + C++ host).
"""
from .lcpc2d import (  # noqa: F401
    FT63, FT127, FT191, FT255, FT253_192, FIELD_NAMES,
    BLAKE3, SHA256, SHA3_256, KECCAK256, digest_name,
    LcpcError, ProverError, VerifierError, FFTError, DeviceError,
    Transcript, CallerTranscript, LcEncoding, LigeroEncoding, RsEncoding, SdigEncoding, LcCommit, LcEvalProof, LcColumn,
    LcBatchEvalProof, BATCH_MAX_TENSORS, collapse_columns_many, collapse_many_chunk,
    collapse_columns, merkle_tree, hash_columns, verify_column_path, verify_column_value,
    n_degree_tests, log2, limbs, num_bits, set_device, device_count, field_random,
    prof_enable, prof_reset, prof_stats, selftest_pool_ordering, selftest_pool_poison,
    SELFTEST_OPS, selftest_fe_dot_kmax, selftest_field_op, selftest_recombine, selftest_recombine63, selftest_twiddle_words, selftest_ntt_rows,
    selftest_spmm, selftest_reed_solomon,
)
# grouped audits of many stored files
from .pos import left_multiply_unencoded_matrices_by_vectors  # noqa: F401,E402
from .pos_files import answer_evaluation_requests  # noqa: F401,E402
# the client's check of those responses, one at a time or grouped
from .pos import client_verify_evaluation, client_verify_evaluations_grouped, verify_group_plan  # noqa: F401,E402
# many small files turned into stored files, or into their roots, in one pass
from .pos import commit_roots_of_files, encode_files_grouped, ingest_plan  # noqa: F401,E402
# the scrubber's triage of many stored files in one pass
from .pos import scrub_files_grouped, scrub_plan  # noqa: F401,E402
from .pos_files import scrub_files  # noqa: F401,E402
# the leg after it: the damaged columns of many stored files recomputed in one pass
from .pos import repair_files_grouped, repair_plan  # noqa: F401,E402
from .pos import locate_files_grouped  # noqa: F401,E402
from .pos_files import repair_files  # noqa: F401,E402
