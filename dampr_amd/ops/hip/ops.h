// Every host entry point of the dampr_hip extension, declared once and
// grouped by the source that implements it.  Each .hip source includes this
// header, so a definition is compiled against its declaration, and
// bindings.cpp binds from it.  Needs ATen only, nothing from HIP.
#pragma once

#include <torch/extension.h>

#include <cstdint>
#include <vector>

// ---- dampr_tfidf.hip: mark scans and the two TF-IDF count kernels
torch::Tensor mark_counts(torch::Tensor text, long mode);
void mark_positions(torch::Tensor text, long mode,
                    torch::Tensor block_offsets, torch::Tensor out);
void tfidf_count(torch::Tensor text, torch::Tensor nl_pos,
                 torch::Tensor tok_start, torch::Tensor seen_keys,
                 torch::Tensor cnt_keys, torch::Tensor cnt_vals,
                 torch::Tensor dict_keys, torch::Tensor dict_vals,
                 long pos_base, long doc_base);
void tfidf_count_docs(torch::Tensor text, torch::Tensor cnt_keys,
                      torch::Tensor cnt_vals, torch::Tensor dict_keys,
                      torch::Tensor dict_vals, long pos_base,
                      torch::Tensor fb_seen, torch::Tensor meta,
                      long ablate);
long tfidf_span_bytes();

// ---- dampr_tables.hip: hash-table ops, idf, token gather, TSV sink
void table_merge(torch::Tensor in_keys, torch::Tensor in_vals,
                 torch::Tensor keys, torch::Tensor vals);
void table_put(torch::Tensor in_keys, torch::Tensor in_vals,
               torch::Tensor keys, torch::Tensor vals);
std::vector<torch::Tensor> table_extract(torch::Tensor keys,
                                         torch::Tensor vals, long n_out);
torch::Tensor table_lookup(torch::Tensor keys, torch::Tensor vals,
                           torch::Tensor query);
torch::Tensor idf(torch::Tensor df, double total);
torch::Tensor gather_tokens(torch::Tensor text, torch::Tensor packed,
                            torch::Tensor offsets, long total_bytes);
torch::Tensor tsv_sizes(torch::Tensor lens, torch::Tensor df,
                        torch::Tensor idf);
torch::Tensor tsv_format(torch::Tensor blob, torch::Tensor tok_off,
                         torch::Tensor lens, torch::Tensor df,
                         torch::Tensor idf, torch::Tensor row_off,
                         long total_bytes);

// ---- dampr_sort.hip: radix sort, fused group-by, merge, join, gather
long rs_span();
torch::Tensor rs_digit_fold(torch::Tensor keys);
torch::Tensor rs_hist(torch::Tensor keys, long shift, long nblocks);
void rs_scatter(torch::Tensor keys, torch::Tensor payload,
                torch::Tensor scanned, long shift, long nblocks,
                torch::Tensor out_k, torch::Tensor out_p);
torch::Tensor seg_count(torch::Tensor keys);
void seg_reduce_fused(torch::Tensor keys, torch::Tensor vals,
                      torch::Tensor tile_base, long op,
                      torch::Tensor out_keys, torch::Tensor out_vals);
void mp_merge(torch::Tensor ka, torch::Tensor pa, torch::Tensor kb,
              torch::Tensor pb, long bias_signed, torch::Tensor out_k,
              torch::Tensor out_p);
void hj_build(torch::Tensor keys_r, torch::Tensor t_keys,
              torch::Tensor t_head, torch::Tensor next);
torch::Tensor hj_count(torch::Tensor keys_l, torch::Tensor t_keys,
                       torch::Tensor t_head, torch::Tensor next,
                       long left_outer);
std::vector<torch::Tensor> hj_emit(torch::Tensor keys_l,
                                   torch::Tensor t_keys,
                                   torch::Tensor t_head,
                                   torch::Tensor next,
                                   torch::Tensor offsets, long total,
                                   long left_outer, long track_matched,
                                   long nr);
void varlen_gather(torch::Tensor blob, torch::Tensor src_off,
                   torch::Tensor lens, torch::Tensor new_offs,
                   torch::Tensor out);

// ---- dampr_strkeys.hip: dictionary encode and byte-order rank of strings
void sv_hash64(torch::Tensor blob, torch::Tensor offs, uint64_t mask,
               torch::Tensor out);
void sv_adjacent_eq(torch::Tensor blob, torch::Tensor offs,
                    torch::Tensor sorted_hash, torch::Tensor perm,
                    torch::Tensor heads, torch::Tensor n_mismatch);
void sv_lex_key(torch::Tensor blob, torch::Tensor offs, torch::Tensor rows,
                long d, torch::Tensor out);
void sv_lex_refine(torch::Tensor grp_sorted, torch::Tensor key_sorted,
                   torch::Tensor heads, torch::Tensor open);

// ---- dampr_filter.hip: numeric row filter and its hash set
long filter_tile();
torch::Tensor filter_count(torch::Tensor keys, torch::Tensor vals,
                           std::vector<int64_t> prog,
                           c10::optional<torch::Tensor> set_k,
                           c10::optional<torch::Tensor> set_v);
void filter_scatter(torch::Tensor keys, torch::Tensor vals,
                    std::vector<int64_t> prog, torch::Tensor block_off,
                    torch::Tensor out_k, torch::Tensor out_v,
                    c10::optional<torch::Tensor> set_k,
                    c10::optional<torch::Tensor> set_v);
long set_capacity(long m);
void set_build(torch::Tensor members, torch::Tensor table);

// ---- dampr_strfilter.hip: string row filter and its string set
long sv_filter_tile();
long sv_filter_max_const();
torch::Tensor sv_filter_count(c10::optional<torch::Tensor> keys,
                              torch::Tensor blob, torch::Tensor offs,
                              std::vector<int64_t> prog,
                              torch::Tensor consts,
                              c10::optional<torch::Tensor> set_k,
                              std::vector<torch::Tensor> sv_set);
void sv_filter_scatter(torch::Tensor keys, torch::Tensor blob,
                       torch::Tensor offs, std::vector<int64_t> prog,
                       torch::Tensor consts, torch::Tensor block_off,
                       torch::Tensor out_k, torch::Tensor out_src,
                       torch::Tensor out_len,
                       c10::optional<torch::Tensor> set_k,
                       std::vector<torch::Tensor> sv_set);
void sv_set_build(torch::Tensor hashes, torch::Tensor slots);
