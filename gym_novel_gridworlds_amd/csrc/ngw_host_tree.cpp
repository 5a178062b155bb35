// ngw_host_tree.cpp - the launches of the tree-search kernels (ngw_tree.inc) behind ngwh::tree_hooks (see ngw_host.h).  Deliberately NOT an
// ngw_abi_*.cpp unit: it is the only host unit that names ngw_tree_*_launch; the entry points and the driver (ngw_abi_tree.cpp) reach the six
// launchers through the pointers filled below when the library is loaded - so the ngw_abi_ units link with or without it.
#include "ngw_host.h"

namespace {

struct Register {
    Register() {
        ngwh::tree_hooks.leaf = ngw_tree_leaf_launch; ngwh::tree_hooks.grow = ngw_tree_grow_launch;
        ngwh::tree_hooks.backup = ngw_tree_backup_launch; ngwh::tree_hooks.reweight = ngw_tree_reweight_launch;
        ngwh::tree_hooks.backup_discount = ngw_tree_backup_discount_launch; ngwh::tree_hooks.reweight16 = ngw_tree_reweight16_launch;
    }
} register_hooks;

}  // namespace
