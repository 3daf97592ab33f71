// Interval join of genes and clusters, and the member-list form of the domain composition (crf_overlap.hip;
// gecco_crf_cluster_overlaps / gecco_crf_domain_composition_members in include/gecco_crf.h).
#pragma once
#include <cstdint>

namespace gecco {

// The argument checks of gecco_crf_cluster_overlaps that need no device: GECCO_CRF_OK or GECCO_CRF_EINVAL with a message.
int overlaps_check(int32_t n_genes, const int32_t *gene_seq, const int64_t *gene_start, const int64_t *gene_end,
                   int32_t n_seqs, const int32_t *cluster_ptr, const int64_t *cluster_start, const int64_t *cluster_end,
                   const uint8_t *label_out, const int32_t *member_ptr_out, int64_t max_members, const int64_t *n_members);
// gecco_crf_cluster_overlaps on checked arguments (the current device is the caller's business).  Synchronous.
int cluster_overlaps(int32_t device, int32_t n_genes, const int32_t *gene_seq, const int64_t *gene_start,
                     const int64_t *gene_end, int32_t n_seqs, const int32_t *cluster_ptr, const int64_t *cluster_start,
                     const int64_t *cluster_end, uint8_t *label_out, int32_t *member_ptr_out, int32_t *member_gene_out,
                     int64_t max_members, int64_t *n_members);

int composition_members_check(const int32_t *member_ptr, int32_t n_clusters, const int32_t *member_gene,
                              const int32_t *dom_ptr, int32_t n_genes, const int32_t *dom_col, const double *dom_weight,
                              int32_t n_cols, const double *comp_out);
// gecco_crf_domain_composition_members on checked arguments with n_clusters > 0 and n_cols > 0.  Synchronous.
int composition_members(int32_t device, const int32_t *member_ptr, int32_t n_clusters, const int32_t *member_gene,
                        const int32_t *dom_ptr, int32_t n_genes, const int32_t *dom_col, const double *dom_weight,
                        int32_t n_cols, int32_t normalize, double *comp_out);

}  // namespace gecco
