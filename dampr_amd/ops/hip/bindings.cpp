// The pybind module of the dampr_hip extension: one m.def per entry point
// declared in ops.h.  Plain C++, nothing from HIP, so touching a binding
// recompiles no kernel.
#include "ops.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    namespace py = pybind11;

    // dampr_tfidf.hip
    m.def("mark_counts", &mark_counts,
          "per-block counts of marks (mode 0=newline, 1=token start)");
    m.def("mark_positions", &mark_positions,
          "write ascending mark positions given exclusive block offsets");
    m.def("tfidf_count", &tfidf_count,
          "tokenize+hash+per-doc-dedupe+df-count in one pass");
    m.def("tfidf_count_docs", &tfidf_count_docs,
          "span-per-wave tokenize+dedupe+count (fast path); counts docs");
    m.def("tfidf_span_bytes", &tfidf_span_bytes,
          "text bytes a wave of tfidf_count_docs owns per visit");

    // dampr_tables.hip
    m.def("table_merge", &table_merge, "add (k,v) pairs into a hash table");
    m.def("table_put", &table_put,
          "insert (k,v) pairs if absent (first writer wins)");
    m.def("table_extract", &table_extract,
          "compact non-empty table slots to (keys, vals, count)");
    m.def("table_lookup", &table_lookup, "probe table for query keys");
    m.def("idf", &idf, "idf = log(1 + total/df)");
    m.def("gather_tokens", &gather_tokens,
          "materialize token byte strings from dict entries");
    m.def("tsv_sizes", &tsv_sizes, "per-row TSV byte sizes");
    m.def("tsv_format", &tsv_format, "format token/df/idf rows as TSV");

    // dampr_sort.hip
    m.def("rs_span", &rs_span,
          "elements per radix block (dampr_sort.hip RS_SPAN)");
    m.def("rs_digit_fold", &rs_digit_fold,
          "AND/OR fold over keys (constant-digit skip detection)");
    m.def("rs_hist", &rs_hist, "radix pass histogram (bin-major)");
    m.def("rs_scatter", &rs_scatter, "stable radix scatter pass");
    m.def("seg_count", &seg_count,
          "segment-start counts per tile (fused group-by, pass 1)");
    m.def("seg_reduce_fused", &seg_reduce_fused,
          "fused boundary-derive + segmented reduce over sorted keys "
          "(op 0=sum,1=min,2=max)");
    m.def("mp_merge", &mp_merge,
          "stable merge-path 2-way merge of sorted (key, payload) runs");
    m.def("hj_build", &hj_build, "hash-join build (chained)");
    m.def("hj_count", &hj_count, "hash-join probe match counts");
    m.def("hj_emit", &hj_emit, "hash-join emit (l,r) row-index pairs");
    m.def("varlen_gather", &varlen_gather,
          "row gather for byte-arena value columns");

    // dampr_strkeys.hip
    m.def("sv_hash64", &sv_hash64,
          "strmix64(row) & mask per row of a byte-arena column");
    m.def("sv_adjacent_eq", &sv_adjacent_eq,
          "segment heads over hash-sorted rows, byte-verified");
    m.def("sv_lex_key", &sv_lex_key,
          "u64 order key of the 7-byte window d of the given rows");
    m.def("sv_lex_refine", &sv_lex_refine,
          "class heads and still-undecided rows over (group, key) order");

    // dampr_filter.hip
    m.def("filter_tile", &filter_tile,
          "rows per filter block (dampr_filter.hip FILTER_TILE)");
    m.def("filter_count", &filter_count,
          "survivors of a clause program per tile (compaction, pass 1)",
          py::arg("keys"), py::arg("vals"), py::arg("prog"),
          py::arg("set_k") = py::none(), py::arg("set_v") = py::none());
    m.def("filter_scatter", &filter_scatter,
          "stable scatter of the surviving rows (compaction, pass 2)",
          py::arg("keys"), py::arg("vals"), py::arg("prog"),
          py::arg("block_off"), py::arg("out_k"), py::arg("out_v"),
          py::arg("set_k") = py::none(), py::arg("set_v") = py::none());
    m.def("set_capacity", &set_capacity,
          "table words for a set of m members (set_table.h)");
    m.def("set_build", &set_build,
          "insert the members' words into a zeroed set table");

    // dampr_strfilter.hip
    m.def("sv_filter_tile", &sv_filter_tile,
          "rows per string-filter block (dampr_strfilter.hip SVF_TILE)");
    m.def("sv_filter_max_const", &sv_filter_max_const,
          "longest string constant of a clause, in bytes");
    m.def("sv_filter_count", &sv_filter_count,
          "survivors of a key/string clause program per tile (pass 1)",
          py::arg("keys"), py::arg("blob"), py::arg("offs"), py::arg("prog"),
          py::arg("consts"), py::arg("set_k") = py::none(),
          py::arg("sv_set") = std::vector<torch::Tensor>());
    m.def("sv_filter_scatter", &sv_filter_scatter,
          "surviving rows' keys, arena offsets and lengths, stable (pass 2)",
          py::arg("keys"), py::arg("blob"), py::arg("offs"), py::arg("prog"),
          py::arg("consts"), py::arg("block_off"), py::arg("out_k"),
          py::arg("out_src"), py::arg("out_len"),
          py::arg("set_k") = py::none(),
          py::arg("sv_set") = std::vector<torch::Tensor>());
    m.def("sv_set_build", &sv_set_build,
          "insert member indices into a zeroed string-set slot table");
}
