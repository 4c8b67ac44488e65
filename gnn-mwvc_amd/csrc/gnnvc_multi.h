// gnnvc_multi.h — several devices behind one handle (gnnvc_create_multi, include/gnnvc.h).  Internal.
//
// The front handle is an ordinary engine on devices[0]; its `multi` member points to the state below, which drives one
// ordinary engine per device — each from a host thread of its own — through the PUBLIC ABI (gnnvc_attach_graph_slice /
// gnnvc_stage_forward_device / gnnvc_pack_rows / gnnvc_push_piece / gnnvc_unpack_pieces): each holds the CSR slice of its rows
// and full-size replicated feature buffers, and after the first and second stage every device pushes the rows it computed,
// packed to their live columns and piece by piece, into every peer's receive buffer (one xGMI link per peer, no ring).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/gnnvc.h"

namespace gnnvc {

struct MultiState;

// generic = gnnvc_create_multi_generic: a model that is a generic stage list under *cfg (never null then; applied to every part's
// engine before its stage list is read) runs the generic route — full rows of any width exchanged after every stage but the
// last; false = gnnvc_create_multi, which refuses such a model.  A model of the trained shape gets the same handle either way.
int multi_create(MultiState **out, const char *model_text, size_t len, const int *devices, int n_devices, bool generic,
                 const gnnvc_generic_config *cfg, std::string &err);
bool multi_is_generic(const MultiState *m);
// a gnnvc_get_info key of the parts' engines, summed over the parts ("generic_heavy_rows" ...)
bool multi_sum_info(MultiState *m, const char *key, long *value);
void multi_destroy(MultiState *m);
int multi_devices(const MultiState *m);
uint32_t multi_vertices(const MultiState *m);
bool multi_has_graph(const MultiState *m);
int multi_set_weight_scale(MultiState *m, float ws);
int multi_set_option(MultiState *m, const char *key, long value);
// exactly one of rowptr64 / rowptr32 is non-null (host arrays: the plain upload, or the staged hand-off's page-locked arrays)
int multi_upload(MultiState *m, uint32_t n, const uint64_t *rowptr64, const uint32_t *rowptr32, const uint32_t *col,
                 const uint32_t *w, const uint32_t *nw, std::string &err);
// d_x / d_scores / d_logits live on devices[0]; complete when it returns (every device's stream is drained)
// audit: the parts audit every stage call of this forward (the front handle counts the calls, option "audit_period"); a part's
// mismatch is returned as GNNVC_ERR_AUDIT once the job has drained, err = "part <p>: " + that part's report
int multi_forward_device(MultiState *m, const float *d_x, float *d_scores, float *d_logits, bool audit, std::string &err);
// gnnvc_get_info keys "audit_*": the parts' counters summed, the first failing part's audit_last_*
bool multi_audit_info(MultiState *m, const char *key, long *value);
int multi_synchronize(MultiState *m);
// rows / entries of part r, wall time of the last forward and of its exchanges as seen by the host
int multi_part_info(const MultiState *m, int part, uint32_t *row_lo, uint32_t *row_hi, uint64_t *entries);
double multi_last_forward_ms(const MultiState *m);
// gnnvc_get_info keys "multi_*" (pieces, packing, bytes shipped per peer and exchange, a part's span of the last forward)
bool multi_get_info(MultiState *m, const char *key, long *value);

}  // namespace gnnvc
