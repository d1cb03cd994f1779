# QPNHip.jl -- `ccall` shim that puts libqpn_hip.so (include/qpn_hip.h) behind the reference's own
# functions for the node-AVI hot path.  SOURCE ONLY: this container has no Julia, so this file has
# never been executed (see INTEGRATION.md); every signature below is checked against the C header
# by hand.  It replaces exactly two bodies in the reference:
#
#   solve_avi(avi::AVI, z0, w)                      src/avi.jl:63-77    (PATHSolver.solve_mcp + check)
#   solve_qp(Q, q, A, l, u; solver=:PATH)           src/qp_processing.jl:12-33
#
# and adds batched entries: solve_avi_batch (many independent AVIs), solve_nodes! (a level of single-node pools), resident
# node records (upload_nodes / solve_nodes!(nodes, ...) / verify_nodes), assemble_pool (combine_gavis) and local_pieces.
#
# Usage from the reference (one line in src/QuadraticProgramNetworks.jl after the includes):
#     include(joinpath(ENV["QPN_HIP_HOME"], "julia", "QPNHip.jl")); using .QPNHip; QPNHip.install!()
module QPNHip

using SparseArrays, LinearAlgebra

const LIB = get(ENV, "QPN_HIP_LIB", joinpath(@__DIR__, "..", "quadraticprogramnetworks.jl_amd", "libqpn_hip.so"))

const QPN_MEM_HOST = Cint(0)
const QPN_SUCCESS = Int32(1)

const QPN_AVI_FLAG_COLD_START = Int32(1)   # include/qpn_hip.h
const QPN_AVI_FLAG_WARM_DUALS = Int32(2)   # n, m <= 32 node solves (mid-size handles after nodes_set_warm!): the multipliers of the incoming z name the active set to start from
struct AviOpts                # qpn_avi_opts, include/qpn_hip.h
    check_tol::Cdouble
    piv_tol::Cdouble
    feas_tol::Cdouble
    comp_tol::Cdouble
    max_pivots::Int32
    flags::Int32
end

const CTX = Ref{Ptr{Cvoid}}(C_NULL)

function ctx()
    if CTX[] == C_NULL
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:qpn_ctx_create, LIB), Cint, (Cint, Ref{Ptr{Cvoid}}), parse(Cint, get(ENV, "QPN_HIP_DEVICE", "0")), h)
        rc == 0 || error("qpn_ctx_create failed: " * unsafe_string(ccall((:qpn_strerror, LIB), Cstring, (Cint,), rc)))
        CTX[] = h[]
        atexit(() -> ccall((:qpn_ctx_destroy, LIB), Cint, (Ptr{Cvoid},), CTX[]))
    end
    CTX[]
end

function default_opts()
    o = Ref(AviOpts(0, 0, 0, 0, 0, 0))
    ccall((:qpn_avi_default_opts, LIB), Cvoid, (Ref{AviOpts},), o)
    o[]
end

"""
    solve_mcp(M, q, l, u, z0) -> (status::Int32, z, info)

Same argument list as `PATHSolver.solve_mcp(M, q, l, u, z0)` at src/avi.jl:64: `M` is the
reference's own `SparseMatrixCSC{Float64,Int32}`; its `colptr/rowval/nzval` (1-based) go to the
library as they are.  Julia owns every array; the callee reads them only during the call.
"""
function solve_mcp(M::SparseMatrixCSC{Float64,Int32}, q::Vector{Float64}, l::Vector{Float64},
                   u::Vector{Float64}, z0::Vector{Float64})
    N = Int32(size(M, 1))
    z = copy(z0)
    status = Ref{Int32}(0); resid = Ref{Cdouble}(0); pivots = Ref{Int32}(0)
    o = Ref(default_opts())
    rc = ccall((:qpn_solve_mcp_csc, LIB), Cint,
               (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ref{Int32}, Ref{Cdouble}, Ref{Int32}, Ref{AviOpts}),
               ctx(), N, M.colptr, M.rowval, M.nzval, q, l, u, z, status, resid, pivots, o)
    rc == 0 || error("qpn_solve_mcp_csc: " * unsafe_string(ccall((:qpn_ctx_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx())))
    (status[], z, (; resid = resid[], pivots = pivots[]))
end

"""
    solve_avi_batch(M, q, l, u, z0; kind=nothing) -> (z, status, resid, pivots, active)

`M` is N×N×batch (Julia column-major = the ABI layout) or N×N (shared, strideM = 0); `q,l,u,z0`
are N×batch.  `kind` (N or N×batch, UInt8) marks GAVI rows (second condition, src/avi.jl:22-24).
"""
function solve_avi_batch(M::Array{Float64}, q::Matrix{Float64}, l::Matrix{Float64}, u::Matrix{Float64},
                         z0::Matrix{Float64}; kind::Union{Nothing,Array{UInt8}} = nothing)
    N, batch = size(q)
    strideM = ndims(M) == 3 ? Int64(N * N) : Int64(0)
    z = copy(z0)
    status = zeros(Int32, batch); resid = zeros(batch); pivots = zeros(Int32, batch); active = zeros(UInt8, N, batch)
    kp = kind === nothing ? Ptr{UInt8}(C_NULL) : pointer(kind)
    sk = kind === nothing ? Int64(0) : (ndims(kind) == 2 ? Int64(N) : Int64(0))
    o = Ref(default_opts())
    GC.@preserve kind begin
        rc = ccall((:qpn_solve_avi_batch, LIB), Cint,
                   (Ptr{Cvoid}, Int32, Int32, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Int64,
                    Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8}, Ref{AviOpts}, Cint),
                   ctx(), Int32(batch), Int32(N), M, strideM, q, l, u, kp, sk, z, status, resid, pivots, active, o, QPN_MEM_HOST)
        rc == 0 || error("qpn_solve_avi_batch failed ($rc)")
    end
    (z, status, resid, pivots, active)
end

"""
    solve_nodes!(x, Qd, R, qd, Ad, B, l, u, w) -> (z, status, resid, pivots, active)

One sweep over `batch` single-node pools: `Qd` n×n×batch, `R` n×p×batch, `qd` n×batch, `Ad` m×n×batch,
`B` m×p×batch, `l,u` m×batch, `w` p (shared) or p×batch.  Each node's reduced KKT system is assembled
on the fly and solved (`qpn_solve_nodes_into`); `z` is (n+m)×batch = [x_d; λ] and the primal blocks are
also written into the columns of `x` (n×batch view of the iterate: the write-back of
src/algorithm.jl:97-101).

`warm = z_prev` (the (n+m)×batch `z` of an earlier sweep over the same nodes; n, m <= 32): its multipliers name the active
set every node starts from (`QPN_AVI_FLAG_WARM_DUALS`).  A node whose hint holds comes back with `pivots == 0`; every other
node is solved cold in the same call.
"""
function solve_nodes!(x::Union{Nothing,StridedMatrix{Float64}}, Qd::Array{Float64,3}, R::Array{Float64,3}, qd::Matrix{Float64},
                      Ad::Array{Float64,3}, B::Array{Float64,3}, l::Matrix{Float64}, u::Matrix{Float64}, w::VecOrMat{Float64};
                      warm::Union{Nothing,Matrix{Float64}} = nothing)
    n, batch = size(qd); m = size(l, 1); p = size(w, 1)
    N = n + m
    warm === nothing || size(warm) == (N, batch) || error("solve_nodes!: warm must be (n+m)×batch")
    z = warm === nothing ? zeros(N, batch) : copy(warm)
    status = zeros(Int32, batch); resid = zeros(batch); pivots = zeros(Int32, batch); active = zeros(UInt8, N, batch)
    o = default_opts()
    o = AviOpts(o.check_tol, o.piv_tol, o.feas_tol, o.comp_tol, o.max_pivots,
                warm === nothing ? o.flags | QPN_AVI_FLAG_COLD_START : o.flags | QPN_AVI_FLAG_WARM_DUALS)
    xp = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    sx = x === nothing ? Int64(0) : Int64(stride(x, 2))
    GC.@preserve x begin
        rc = ccall((:qpn_solve_nodes_into, LIB), Cint,
                   (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8},
                    Ref{AviOpts}, Cint, Ptr{Cdouble}, Int64),
                   ctx(), Int32(batch), Int32(n), Int32(m), Int32(p), Qd, R, qd, Ad, B, l, u, w, ndims(w) == 1 ? Int64(0) : Int64(p),
                   z, status, resid, pivots, active, Ref(o), QPN_MEM_HOST, xp, sx)
        rc == 0 || error("qpn_solve_nodes_into failed ($rc)")
    end
    (z, status, resid, pivots, active)
end

# ---- resident node records: upload once, sweep many times (qpn_nodes_*, include/qpn_hip.h) ---------------------------
const QPN_NODE_QD, QPN_NODE_R, QPN_NODE_Q, QPN_NODE_AD, QPN_NODE_B, QPN_NODE_L, QPN_NODE_U = Int32.(0:6)

"""
    nodes = upload_nodes(Qd, R, qd, Ad, B, l, u)      # arrays as in solve_nodes!; the library keeps its own copy in HBM
    (z, status, resid, pivots, active) = solve_nodes!(nodes, x, w)       # one sweep: only w goes up, only outputs come down
    (solution, lambda, path) = verify_nodes(nodes, xd, w)
    update_nodes!(nodes, QPN_NODE_L, l_new); free_nodes!(nodes)

The outer loop (src/algorithm.jl:13-117) sweeps the same nodes with new parameters every iteration: with the records
resident the PCIe traffic per sweep is w in and the requested outputs out (`want_z = false` returns only the statuses and
the primal blocks in `x`), instead of 22 KB per node in.  The handle also remembers whether any of its nodes needs the
general (pivoting) kernel and keeps their longest-first schedule.
"""
mutable struct Nodes
    h::Ptr{Cvoid}
    batch::Int; n::Int; m::Int; p::Int
end

function upload_nodes(Qd::Array{Float64,3}, R::Array{Float64,3}, qd::Matrix{Float64}, Ad::Array{Float64,3}, B::Array{Float64,3},
                      l::Matrix{Float64}, u::Matrix{Float64})
    n, batch = size(qd); m = size(l, 1); p = size(R, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:qpn_nodes_upload, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Cint, Ref{Ptr{Cvoid}}),
               ctx(), Int32(batch), Int32(n), Int32(m), Int32(p), Qd, R, qd, Ad, B, l, u, QPN_MEM_HOST, h)
    rc == 0 || error("qpn_nodes_upload failed ($rc)")
    nodes = Nodes(h[], batch, n, m, p)
    finalizer(free_nodes!, nodes)
    nodes
end

function free_nodes!(nodes::Nodes)
    nodes.h == C_NULL && return nothing
    ccall((:qpn_nodes_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), nodes.h)
    nodes.h = C_NULL
    nothing
end

function update_nodes!(nodes::Nodes, field::Int32, data::Array{Float64})
    rc = ccall((:qpn_nodes_update, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cdouble}, Cint), ctx(), nodes.h, field, data, QPN_MEM_HOST)
    rc == 0 || error("qpn_nodes_update failed ($rc)")
    nothing
end

# Opt a handle of the mid-size classes (n, m <= 128, one of them > 32) in to the warm start (`on = true`) or out of it: with it on,
# solve_nodes!(nodes, w; warm = z_prev) runs the warm kernel ahead of the cold one.  On a handle of another shape nothing changes.
function nodes_set_warm!(nodes::Nodes, on::Bool = true)
    rc = ccall((:qpn_nodes_set_warm, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), ctx(), nodes.h, Int32(on))
    rc == 0 || error("qpn_nodes_set_warm failed ($rc)")
    nothing
end

# warm = the z of an earlier sweep over the handle's nodes: QPN_AVI_FLAG_WARM_DUALS, as in solve_nodes! above (z comes back).
# Handles of the mid-size classes take it after nodes_set_warm!(nodes).
# Handles of large symmetric nodes (64 < n <= 256, m <= 256) take it too after set_option!(QPN_OPT_WARM_BIG, 1): the hint seeds
# block principal pivoting, `pivots == n` says that it held, and a wrong hint costs rounds, never the result; without the option
# the hint is ignored in that class.
function solve_nodes!(nodes::Nodes, x::Union{Nothing,StridedMatrix{Float64}}, w::VecOrMat{Float64}; want_z::Bool = true,
                      warm::Union{Nothing,Matrix{Float64}} = nothing)
    N = nodes.n + nodes.m; batch = nodes.batch
    warm === nothing || size(warm) == (N, batch) || error("solve_nodes!: warm must be (n+m)×batch")
    want_z = want_z || warm !== nothing
    z = warm !== nothing ? copy(warm) : (want_z ? zeros(N, batch) : nothing)
    o = default_opts()
    oref = Ref(AviOpts(o.check_tol, o.piv_tol, o.feas_tol, o.comp_tol, o.max_pivots, o.flags | QPN_AVI_FLAG_WARM_DUALS))
    status = zeros(Int32, batch); resid = zeros(batch); pivots = zeros(Int32, batch)
    active = want_z ? zeros(UInt8, N, batch) : nothing
    xp = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    sx = x === nothing ? Int64(0) : Int64(stride(x, 2))
    GC.@preserve x z active oref begin
        optr = warm === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(Base.unsafe_convert(Ptr{AviOpts}, oref))
        rc = ccall((:qpn_solve_nodes_h, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8},
                    Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64),
                   ctx(), nodes.h, w, ndims(w) == 1 ? Int64(0) : Int64(nodes.p),
                   want_z ? pointer(z) : Ptr{Cdouble}(C_NULL), status, resid, pivots, want_z ? pointer(active) : Ptr{UInt8}(C_NULL),
                   optr, QPN_MEM_HOST, xp, sx)
        rc == 0 || error("qpn_solve_nodes_h failed ($rc)")
    end
    (z, status, resid, pivots, active)
end

# A sweep over the nodes `idx` names (1-based, distinct, any order; qpn_solve_nodes_subset_h): column s of every array belongs to
# node idx[s] -- w is p×count (or a shared vector), warm and the returned z and active are (n+m)×count, x (n rows or more,
# count columns) receives the primal blocks.  Column s equals what solve_nodes! returns for node idx[s] given the same w column
# (and hint), bit for bit.  Handles with n, m <= 128 solve only the listed nodes and their state does not move; larger records
# run a full sweep and return the listed columns.
function solve_nodes_subset!(nodes::Nodes, idx::Vector{<:Integer}, x::Union{Nothing,StridedMatrix{Float64}}, w::VecOrMat{Float64};
                             want_z::Bool = true, warm::Union{Nothing,Matrix{Float64}} = nothing)
    N = nodes.n + nodes.m; count = length(idx)
    count <= nodes.batch || error("solve_nodes_subset!: more entries than nodes")
    ndims(w) == 1 || size(w, 2) == count || error("solve_nodes_subset!: w must be p×count")
    warm === nothing || size(warm) == (N, count) || error("solve_nodes_subset!: warm must be (n+m)×count")
    x === nothing || size(x, 2) == count || error("solve_nodes_subset!: x must have count columns")
    idx0 = Int32.(idx .- 1)
    want_z = want_z || warm !== nothing
    z = warm !== nothing ? copy(warm) : (want_z ? zeros(N, count) : nothing)
    o = default_opts()
    oref = Ref(AviOpts(o.check_tol, o.piv_tol, o.feas_tol, o.comp_tol, o.max_pivots, o.flags | QPN_AVI_FLAG_WARM_DUALS))
    status = zeros(Int32, count); resid = zeros(count); pivots = zeros(Int32, count)
    active = want_z ? zeros(UInt8, N, count) : nothing
    xp = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    sx = x === nothing ? Int64(0) : Int64(stride(x, 2))
    GC.@preserve x z active oref begin
        optr = warm === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(Base.unsafe_convert(Ptr{AviOpts}, oref))
        rc = ccall((:qpn_solve_nodes_subset_h, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32},
                    Ptr{UInt8}, Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64),
                   ctx(), nodes.h, Int32(count), idx0, w, ndims(w) == 1 ? Int64(0) : Int64(nodes.p),
                   want_z ? pointer(z) : Ptr{Cdouble}(C_NULL), status, resid, pivots, want_z ? pointer(active) : Ptr{UInt8}(C_NULL),
                   optr, QPN_MEM_HOST, xp, sx)
        rc == 0 || error("qpn_solve_nodes_subset_h failed ($rc)")
    end
    (z, status, resid, pivots, active)
end

"""
    convexity_nodes(Qd, Ad, eq; tol=1e-6) -> (convex, min_eig, null_dim)

check_qp_convexity (src/qp_processing.jl:39-55) for a batch: Qd [n, n, batch], Ad [m, n, batch] (Julia's column-major
arrays are the ABI layout as they are), eq [m, batch] (1 = implicit equality row, from `implicit_bounds`).
"""
function convexity_nodes(Qd::Array{Float64,3}, Ad::Array{Float64,3}, eq::Matrix{UInt8}; tol::Float64 = 1e-6)
    n, batch = size(Qd, 1), size(Qd, 3)
    m = size(Ad, 1)
    convex = zeros(Int32, batch); min_eig = zeros(batch); null_dim = zeros(Int32, batch)
    rc = ccall((:qpn_convexity_nodes, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Cdouble, Ptr{Int32}, Ptr{Cdouble},
                Ptr{Int32}, Cint),
               ctx(), batch, n, m, Qd, Ad, eq, tol, convex, min_eig, null_dim, QPN_MEM_HOST)
    rc == 0 || error("qpn_convexity_nodes failed ($rc)")
    (convex, min_eig, null_dim)
end

"""
    multiplier_vertices(Ad, g, cls, lam0, V; max_bases=64V, tol=1e-9, feas=1e-6) -> (verts, count, status)

Vertices of the multiplier sets {lambda : Ad' lambda = g, per-row class} of a batch (qpn_multiplier_vertices): Ad [m, n, batch],
g [n, batch], cls [m, batch] (0 >= 0, 1 <= 0, 2 free, 3 = 0), lam0 [m, batch] the start.  verts [m, V, batch], count and
status [batch] (0 complete, 1 vertex budget, 2 basis budget, 3 empty, 4 no vertex).
"""
function multiplier_vertices(Ad::Array{Float64,3}, g::Matrix{Float64}, cls::Matrix{UInt8}, lam0::Matrix{Float64}, V::Integer;
                             max_bases::Integer = 64V, tol::Float64 = 1e-9, feas::Float64 = 1e-6)
    m, n, batch = size(Ad)
    verts = zeros(m, V, batch); count = zeros(Int32, batch); status = zeros(Int32, batch)
    rc = ccall((:qpn_multiplier_vertices, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{Cdouble}, Int32, Int32, Cdouble, Cdouble,
                Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Cint),
               ctx(), batch, n, m, Ad, g, cls, lam0, V, max_bases, tol, feas, verts, count, status, QPN_MEM_HOST)
    rc == 0 || error("qpn_multiplier_vertices failed ($rc)")
    (verts, count, status)
end

"""
    recipe_filter(masks, K, vrow_of, first_of) -> keep

qpn_recipe_filter: masks [N, rows], K [N, pieces] (codes 1..8), vrow_of [pieces] and first_of [rows] (0-based rows, Int32).
keep[t] = 0 when an earlier row of the recipe's item holds every one of its codes.
"""
function recipe_filter(masks::Matrix{UInt8}, K::Matrix{UInt8}, vrow_of::Vector{Int32}, first_of::Vector{Int32})
    N, rows = size(masks); pieces = size(K, 2)
    keep = zeros(UInt8, pieces)
    rc = ccall((:qpn_recipe_filter, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Cint),
               ctx(), pieces, rows, N, masks, K, vrow_of, first_of, keep, QPN_MEM_HOST)
    rc == 0 || error("qpn_recipe_filter failed ($rc)")
    keep
end

"""
    interior_members(A, l, u; delta=1e-2) -> (x, ok, status)

One member per polyhedron {x : l <= A x <= u}, well inside its inequality rows (qpn_interior_members: the slack program of
`exemplar` with a proximal term, equality rows kept; the node records are made on the device).  A [r, d, batch] (Julia's
column-major arrays are the ABI layout as they are), l, u [r, batch].  x [d, batch] (meaningful where ok), ok [batch] (1 = a
member), status [batch] the node solver's.
"""
function interior_members(A::Array{Float64,3}, l::Matrix{Float64}, u::Matrix{Float64}; delta::Float64 = 1e-2)
    r, d, batch = size(A)
    eq = isfinite.(l) .& (l .== u)
    ne = Int32(maximum(sum(eq, dims = 1); init = 0))
    nlo = Int32(maximum(sum(.!eq .& isfinite.(l), dims = 1); init = 0))
    nhi = Int32(maximum(sum(.!eq .& isfinite.(u), dims = 1); init = 0))
    x = zeros(d, batch); ok = zeros(UInt8, batch); status = zeros(Int32, batch)
    rc = ccall((:qpn_interior_members, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int32, Int32, Int32, Ptr{Cdouble},
                Ptr{UInt8}, Ptr{Int32}, Cint),
               ctx(), batch, r, d, A, l, u, delta, ne, nlo, nhi, x, ok, status, QPN_MEM_HOST)
    rc == 0 || error("qpn_interior_members failed ($rc)")
    (x, ok, status)
end

"""
    assemble_interior_nodes(A, l, u, ne, nlo, nhi; delta=1e-2) -> (Qd, qd, Ad, lo, uo, flag)

The node records interior_members solves (qpn_assemble_interior_nodes): Qd [nf, nf, batch], qd [nf, batch], Ad [mp, nf, batch],
lo, uo [mp, batch] with nf = d + 1 + ne, mp = max(16, nlo + nhi rounded up to 16); flag [batch] = 1 for an item with more rows
of a class than slots (its record is that of a polyhedron without rows).
"""
function assemble_interior_nodes(A::Array{Float64,3}, l::Matrix{Float64}, u::Matrix{Float64}, ne::Integer, nlo::Integer,
                                 nhi::Integer; delta::Float64 = 1e-2)
    r, d, batch = size(A)
    nf = d + 1 + ne
    mp = max(16, cld(nlo + nhi, 16) * 16)
    Qd = zeros(nf, nf, batch); qd = zeros(nf, batch); Ad = zeros(mp, nf, batch); lo = zeros(mp, batch); uo = zeros(mp, batch)
    flag = zeros(UInt8, batch)
    rc = ccall((:qpn_assemble_interior_nodes, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int32, Int32, Int32, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Cint),
               ctx(), batch, r, d, A, l, u, delta, ne, nlo, nhi, Qd, qd, Ad, lo, uo, flag, QPN_MEM_HOST)
    rc == 0 || error("qpn_assemble_interior_nodes failed ($rc)")
    (Qd, qd, Ad, lo, uo, flag)
end

"""
    members_outside(Aj, lj, uj, X, pi, pj; t=1e-5) -> out

qpn_members_outside: out[q] = 1 when member X[:, pi[q]] violates a row of piece pj[q] (Aj [rj, d, Bj], lj, uj [rj, Bj]) by more
than t.  pi, pj are 1-based here.
"""
function members_outside(Aj::Array{Float64,3}, lj::Matrix{Float64}, uj::Matrix{Float64}, X::Matrix{Float64}, pi::Vector{<:Integer},
                         pj::Vector{<:Integer}; t::Float64 = 1e-5)
    rj, d, Bj = size(Aj)
    size(X, 1) == d || error("members_outside: X must have d rows")
    pairs = length(pi)
    pi0 = Int32.(pi .- 1); pj0 = Int32.(pj .- 1)
    out = zeros(UInt8, pairs)
    rc = ccall((:qpn_members_outside, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Int32, Ptr{Int32},
                Ptr{Int32}, Cdouble, Ptr{UInt8}, Cint),
               ctx(), pairs, d, rj, Aj, lj, uj, Bj, X, size(X, 2), pi0, pj0, t, out, QPN_MEM_HOST)
    rc == 0 || error("qpn_members_outside failed ($rc)")
    out
end

"""
    members_outside_lists(Aj, lj, uj, X, ok, list_ptr, list_mem, list_of, self_pos; t=1e-5) -> (bits, undecided, word_ptr)

qpn_members_outside_lists: every member of a list against every piece of the same list, the pairs enumerated on the device.  One
pack of second pieces (Aj [rj, d, Bj], lj, uj [rj, Bj]); members X [d, Bi] with the flags ok [Bi] of interior_members; the lists
as a CSR: list_ptr [lists + 1] (0-based offsets, as the ABI has them) and list_mem (1-based columns of X, 0 = that piece has no
member); list_of [Bj] (1-based list of piece j) and self_pos [Bj] (its own 1-based position there).  Piece j owns the words
bits[word_ptr[j] + 1 : word_ptr[j + 1]] (word_ptr is made here, ceil(k / 32) words for a list of k): bit (s - 1) & 31 of word
(s - 1) >> 5 is 1 when the member at position s != self_pos[j] exists, is ok and violates a row of piece j by more than t.
undecided[j] counts the positions other than its own whose bit is 0: the pairs still to be put to an LP.
"""
function members_outside_lists(Aj::Array{Float64,3}, lj::Matrix{Float64}, uj::Matrix{Float64}, X::Matrix{Float64}, ok::Vector{UInt8},
                               list_ptr::Vector{<:Integer}, list_mem::Vector{<:Integer}, list_of::Vector{<:Integer},
                               self_pos::Vector{<:Integer}; t::Float64 = 1e-5)
    rj, d, Bj = size(Aj)
    size(X, 1) == d || error("members_outside_lists: X must have d rows")
    Bi = size(X, 2)
    length(ok) == Bi || error("members_outside_lists: one ok flag per member")
    lists = length(list_ptr) - 1
    lp = Int32.(list_ptr); lm = Int32.(list_mem .- 1); lo = Int32.(list_of .- 1); sp = Int32.(self_pos .- 1)
    word_ptr = zeros(Int64, Bj + 1)
    for j in 1:Bj
        1 <= list_of[j] <= lists || error("members_outside_lists: list_of out of range")
        k = lp[list_of[j] + 1] - lp[list_of[j]]
        word_ptr[j + 1] = word_ptr[j] + cld(k, 32)
    end
    bits = zeros(UInt32, word_ptr[end]); undecided = zeros(Int32, Bj)
    rc = ccall((:qpn_members_outside_lists, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{UInt8}, Int32, Int32,
                Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Cdouble, Ptr{UInt32}, Ptr{Int32}, Cint),
               ctx(), d, rj, Aj, lj, uj, Bj, X, ok, Bi, lists, lp, lm, lo, sp, word_ptr, t, bits, undecided, QPN_MEM_HOST)
    rc == 0 || error("qpn_members_outside_lists failed ($rc)")
    (bits, undecided, word_ptr)
end

"""
    assemble_parent_nodes(form, ne, m, p, sQd, sR, sqd, sAd, sB, sl, su, mb_true, piece_desc, pA, pl, pu, map_off, map_data,
                          parent_of, piece_of, map_of) -> (Qd, R, qd, Ad, B, l, u, err)

qpn_assemble_parent_nodes: the records of inner nodes, an item being one parent under one choice of its children's pieces (the
constraint stack [base; child pieces], src/qp_processing.jl:62-66), from a static store sQd [n0, n0, parents], sR [n0, ps,
parents], sqd [n0, parents], sAd [mb, n0, parents], sB [mb, ps, parents], sl, su [mb, parents], mb_true [parents]; a piece pool
piece_desc [4, pieces] = (row0, rows, c, off) with pA (row-major per piece), pl, pu; column maps map_off [maps + 1], map_data;
and items parent_of [items], piece_of, map_of [8, items].  Every index and offset is 0-BASED, as the ABI has it (piece_of -1 = an
empty slot, a map entry -1 = a variable the parent does not read).  form 0: the verify form (n = n0); form 1: the solve form,
the ne equality rows in the free block (n = n0 + ne).  Qd [n, n, items], R [n, p, items], qd [n, items], Ad [m, n, items],
B [m, p, items], l, u [m, items]; a bad item is an error (include/qpn_hip.h lists the err words).
"""
function assemble_parent_nodes(form::Integer, ne::Integer, m::Integer, p::Integer, sQd::Array{Float64,3}, sR::Array{Float64,3},
                               sqd::Matrix{Float64}, sAd::Array{Float64,3}, sB::Array{Float64,3}, sl::Matrix{Float64},
                               su::Matrix{Float64}, mb_true::Vector{Int32}, piece_desc::Matrix{Int32}, pA::Vector{Float64},
                               pl::Vector{Float64}, pu::Vector{Float64}, map_off::Vector{Int32}, map_data::Vector{Int32},
                               parent_of::Vector{Int32}, piece_of::Matrix{Int32}, map_of::Matrix{Int32})
    n0, parents = size(sqd)
    ps = size(sR, 2); mb = size(sl, 1)
    items = length(parent_of); pieces = size(piece_desc, 2); maps = length(map_off) - 1
    (size(piece_desc, 1) == 4 && size(piece_of) == (8, items) && size(map_of) == (8, items) && maps >= 0) ||
        error("assemble_parent_nodes: inconsistent shapes")
    n = n0 + (form == 0 ? 0 : ne)
    Qd = zeros(n, n, items); R = zeros(n, p, items); qd = zeros(n, items); Ad = zeros(m, n, items); B = zeros(m, p, items)
    l = zeros(m, items); u = zeros(m, items); err = zeros(Int32, items)
    rc = ccall((:qpn_assemble_parent_nodes, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Int32, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Cint),
               ctx(), items, form, n0, ne, m, p, parents, mb, ps, sQd, sR, sqd, sAd, sB, sl, su, mb_true, pieces, piece_desc,
               length(pl), length(pA), pA, pl, pu, maps, map_off, length(map_data), map_data, parent_of, piece_of, map_of,
               Qd, R, qd, Ad, B, l, u, err, QPN_MEM_HOST)
    rc == 0 || error("qpn_assemble_parent_nodes failed ($rc)")
    (Qd, R, qd, Ad, B, l, u, err)
end

"""
    solve_lps(A, l, u, poly_of; cost=nothing, obj_row=nothing, obj_sign=nothing, max_iters=0)
        -> (status, x, obj, lambda, ray, iters)

qpn_solve_lps: the LPs of `exemplar`, `isempty`, `issubset` and `implicit_bounds` (src/sets.jl:591-713, :376-407) as jobs over
shared polyhedra A [r, d, polys], l, u [r, polys].  Job t minimises cost[:, t]'x over polyhedron poly_of[t] or, without `cost`,
obj_sign[t] times row obj_row[t] of it (poly_of and obj_row are 1-based here).  status: 1 optimal, 2 infeasible (lambda is a
Farkas vector), 3 unbounded (x + t ray stays feasible and c'ray < 0), 4 iteration limit, 5 failure.
"""
function solve_lps(A::Array{Float64,3}, l::Matrix{Float64}, u::Matrix{Float64}, poly_of::Vector{<:Integer};
                   cost::Union{Nothing,Matrix{Float64}} = nothing, obj_row::Union{Nothing,Vector{<:Integer}} = nothing,
                   obj_sign::Union{Nothing,Vector{<:Integer}} = nothing, max_iters::Integer = 0)
    r, d, polys = size(A)
    jobs = length(poly_of)
    cost === nothing && (obj_row === nothing || obj_sign === nothing) && error("solve_lps: give cost, or obj_row and obj_sign")
    po = Int32.(poly_of .- 1)
    orow = cost === nothing ? Int32.(obj_row .- 1) : Int32[]
    osg = cost === nothing ? Int32.(obj_sign) : Int32[]
    opts = Ref((1e-9, 1e-9, 1e-9, 1e-6, Int32(max_iters), Int32(0)))      # qpn_lp_opts
    status = zeros(Int32, jobs); x = zeros(d, jobs); obj = zeros(jobs); lam = zeros(r, jobs); ray = zeros(d, jobs)
    iters = zeros(Int32, jobs)
    rc = ccall((:qpn_solve_lps, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32},
                Ptr{Int32}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Cint),
               ctx(), polys, r, d, A, l, u, jobs, po, cost === nothing ? C_NULL : cost, cost === nothing ? orow : C_NULL,
               cost === nothing ? osg : C_NULL, opts, status, x, obj, lam, ray, iters, QPN_MEM_HOST)
    rc == 0 || error("qpn_solve_lps failed ($rc)")
    (status, x, obj, lam, ray, iters)
end

"""
    issubset_pairs(A1, l1, u1, A2, l2, u2, pi, pj; tol=1e-6, max_iters=0) -> (sub, how, bound, val, lps, iters)

qpn_issubset_pairs: `issubset(P1, P2)` (src/sets.jl:376-407) for pairs of pieces, one job per pair: first piece pi[q] of
A1 [r1, d, B1], l1, u1 [r1, B1] against second piece pj[q] of A2 [r2, d, B2], l2, u2 [r2, B2] (pi, pj are 1-based here).  The crash
and phase 1 over P1 run once, then the finite bounds of P2 are tried one after the other until one refutes.  sub[q] = 1 for how = 0
(holds) and 6 (P1 empty); how 1: refuted by the current vertex, 2: by a certified optimum, 3: a bound's objective is unbounded,
4: iteration limit, 5: failure.  bound: 2 i + side (0-based row i of P2, side 0 = lower, 1 = upper) of the bound that decided, -1
without one; val: the value that decided; lps: solves started; iters: all their steps.
"""
function issubset_pairs(A1::Array{Float64,3}, l1::Matrix{Float64}, u1::Matrix{Float64}, A2::Array{Float64,3}, l2::Matrix{Float64},
                        u2::Matrix{Float64}, pi::Vector{<:Integer}, pj::Vector{<:Integer}; tol::Float64 = 1e-6, max_iters::Integer = 0)
    r1, d, B1 = size(A1)
    r2, d2, B2 = size(A2)
    d2 == d || error("issubset_pairs: A1 and A2 must have the same number of columns")
    size(l1) == (r1, B1) && size(u1) == (r1, B1) && size(l2) == (r2, B2) && size(u2) == (r2, B2) || error("issubset_pairs: inconsistent shapes")
    pairs = length(pi)
    length(pj) == pairs || error("issubset_pairs: pi and pj must have the same length")
    pi0 = Int32.(pi .- 1); pj0 = Int32.(pj .- 1)
    opts = Ref((1e-9, 1e-9, 1e-9, 1e-6, Int32(max_iters), Int32(0)))      # qpn_lp_opts
    sub = zeros(UInt8, pairs); how = zeros(Int32, pairs); bound = zeros(Int32, pairs); val = zeros(pairs)
    lps = zeros(Int32, pairs); iters = zeros(Int32, pairs)
    rc = ccall((:qpn_issubset_pairs, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Int32, Ptr{Int32}, Ptr{Int32}, Cdouble, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble},
                Ptr{Int32}, Ptr{Int32}, Cint),
               ctx(), d, B1, r1, A1, l1, u1, B2, r2, A2, l2, u2, pairs, pi0, pj0, tol, opts, sub, how, bound, val, lps, iters, QPN_MEM_HOST)
    rc == 0 || error("qpn_issubset_pairs failed ($rc)")
    (sub, how, bound, val, lps, iters)
end

"""
    implicit_bounds(polys; tol=1e-4, all_extremes=false, max_iters=0) -> [(implicitly_equality, vals), ...]

qpn_implicit_bounds: `implicit_bounds(poly; tol)` (src/sets.jl:660-713) for a list of polyhedra `(A, l, u)` (A [r, d], l, u [r]), one
job per polyhedron: the crash and phase 1 once, then the rows that are no explicit equalities from the last, the minimum and the
maximum of each from the basis the previous solve left; a row whose values at two points the solves ended at differ by more than tol
needs no LP.  Polyhedra of one shape go up in one call.  Returns per polyhedron `implicitly_equality::Vector{Bool}` and
`vals::Vector{Float64}` (Inf where the row is no equality), as the reference does.  An empty polyhedron raises "Empty set" like the
reference (:688-690); any other status names the polyhedron and the row whose solve ended it.
"""
function implicit_bounds(polys::Vector{<:Tuple{Matrix{Float64},Vector{Float64},Vector{Float64}}}; tol::Float64 = 1e-4,
                         all_extremes::Bool = false, max_iters::Integer = 0)
    out = Vector{Tuple{Vector{Bool},Vector{Float64}}}(undef, length(polys))
    packs = Dict{Tuple{Int,Int},Vector{Int}}()
    for (k, (A, l, u)) in enumerate(polys)
        length(l) == size(A, 1) && length(u) == size(A, 1) || error("implicit_bounds: inconsistent shapes (polyhedron $k)")
        push!(get!(packs, size(A), Int[]), k)
    end
    opts = Ref((1e-9, 1e-9, 1e-9, 1e-6, Int32(max_iters), Int32(0)))      # qpn_lp_opts
    empty = Int[]
    for ((r, d), members) in sort(collect(packs))
        n = length(members)
        A = Array{Float64,3}(undef, r, d, n); l = Matrix{Float64}(undef, r, n); u = Matrix{Float64}(undef, r, n)
        for (t, k) in enumerate(members)
            A[:, :, t] = polys[k][1]; l[:, t] = polys[k][2]; u[:, t] = polys[k][3]
        end
        status = zeros(Int32, n); fail_row = zeros(Int32, n); eq = zeros(UInt8, r, n); vals = zeros(r, n)
        rc = ccall((:qpn_implicit_bounds, LIB), Cint,
                   (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int32, Ptr{Cvoid}, Ptr{Int32},
                    Ptr{Int32}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Cint),
                   ctx(), n, r, d, A, l, u, tol, Int32(all_extremes ? 1 : 0), opts, status, fail_row, eq, vals, C_NULL, C_NULL, C_NULL,
                   C_NULL, C_NULL, QPN_MEM_HOST)
        rc == 0 || error("qpn_implicit_bounds failed ($rc)")
        for (t, k) in enumerate(members)
            if status[t] == 1
                push!(empty, k)
            elseif status[t] != 0
                error("implicit_bounds: status $(status[t]) on polyhedron $k, row $(fail_row[t] + 1)")
            end
            out[k] = (eq[:, t] .!= 0, vals[:, t])
        end
    end
    isempty(empty) || error("Empty set (polyhedron $(minimum(empty)))")
    out
end

"""
    irredundant_bounds(polys; tol=1e-8, max_iters=0) -> [(l, u, status), ...]

qpn_irredundant_bounds: the bounds of a list of polyhedra `(A, l, u)` (A [r, d], l, u [r]) that their other bounds imply, one job per
polyhedron: the crash and phase 1 once, then the finite bounds of the rows from the last, each relaxed and its row minimised
(maximised) from the basis the previous solve left; a bound the optimum does not pass by more than tol * max(1, |bound|) is
removed and stays removed for the later tests.  What the reference's `project` (src/sets.jl:501-523) returns as facets.  Polyhedra of
one shape go up in one call.  Returns per polyhedron the bounds with every removed one at -Inf / Inf and the status (0 OK; 1 empty, 2
iteration limit, 3 failure: the bounds come back as given).
"""
function irredundant_bounds(polys::Vector{<:Tuple{Matrix{Float64},Vector{Float64},Vector{Float64}}}; tol::Float64 = 1e-8,
                            max_iters::Integer = 0)
    out = Vector{Tuple{Vector{Float64},Vector{Float64},Int}}(undef, length(polys))
    packs = Dict{Tuple{Int,Int},Vector{Int}}()
    for (k, (A, l, u)) in enumerate(polys)
        length(l) == size(A, 1) && length(u) == size(A, 1) || error("irredundant_bounds: inconsistent shapes (polyhedron $k)")
        push!(get!(packs, size(A), Int[]), k)
    end
    opts = Ref((1e-9, 1e-9, 1e-9, 1e-6, Int32(max_iters), Int32(0)))      # qpn_lp_opts
    for ((r, d), members) in sort(collect(packs))
        n = length(members)
        A = Array{Float64,3}(undef, r, d, n); l = Matrix{Float64}(undef, r, n); u = Matrix{Float64}(undef, r, n)
        for (t, k) in enumerate(members)
            A[:, :, t] = polys[k][1]; l[:, t] = polys[k][2]; u[:, t] = polys[k][3]
        end
        status = zeros(Int32, n); lr = zeros(r, n); ur = zeros(r, n)
        rc = ccall((:qpn_irredundant_bounds, LIB), Cint,
                   (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cvoid}, Ptr{Int32},
                    Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Cint),
                   ctx(), n, r, d, A, l, u, tol, opts, status, C_NULL, lr, ur, C_NULL, C_NULL, C_NULL, C_NULL, QPN_MEM_HOST)
        rc == 0 || error("qpn_irredundant_bounds failed ($rc)")
        for (t, k) in enumerate(members)
            out[k] = (lr[:, t], ur[:, t], Int(status[t]))
        end
    end
    out
end

"""
    exemplar_polys(A, l, u; open_lo=nothing, open_hi=nothing, tol=1e-2, slack_cap=1.0, max_iters=0)
        -> (empty, how, eps, x, row, lambda, iters)

qpn_exemplar_polys: `exemplar(poly; tol)` / `isempty` (src/sets.jl:591-655) for polyhedra of one shape whose bounds may be open, one
job per polyhedron: A [n, d, polys], l, u [n, polys], open_lo, open_hi [n, polys] (Bool or UInt8; nothing: closed).  The job expands
the slack LP min eps s.t. A x + eps >= l, -A x + eps >= -u, eps >= -slack_cap on the device, solves it and applies the reference's
rule to eps and the multipliers of the open, finite bounds.  how: 0 member (eps <= -tol), 1 member in the band, 2 empty (eps > tol),
3 empty by an active open bound (row: 2 i + side, 0-based row i, side 0 = lower, 1 = upper; -1 otherwise), 4 iteration limit, 5
failure (both without an answer: empty = 0, eps = NaN).  x [d, polys]: a member, zeros when empty or unanswered; lambda [2 n + 1,
polys]: the multipliers of the slack LP's rows.  n <= 511, d <= 255.
"""
function exemplar_polys(A::Array{Float64,3}, l::Matrix{Float64}, u::Matrix{Float64};
                        open_lo::Union{Nothing,AbstractMatrix} = nothing, open_hi::Union{Nothing,AbstractMatrix} = nothing,
                        tol::Float64 = 1e-2, slack_cap::Float64 = 1.0, max_iters::Integer = 0)
    n, d, polys = size(A)
    size(l) == (n, polys) && size(u) == (n, polys) || error("exemplar_polys: inconsistent shapes")
    flags(o) = o === nothing ? nothing : (size(o) == (n, polys) || error("exemplar_polys: inconsistent shapes"); Matrix{UInt8}(o .!= 0))
    olo = flags(open_lo); ohi = flags(open_hi)
    opts = Ref((1e-9, 1e-9, 1e-9, 1e-6, Int32(max_iters), Int32(0)))      # qpn_lp_opts
    empty = zeros(UInt8, polys); how = zeros(Int32, polys); eps = zeros(polys); x = zeros(d, polys); row = zeros(Int32, polys)
    lam = zeros(2n + 1, polys); iters = zeros(Int32, polys)
    rc = ccall((:qpn_exemplar_polys, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Cdouble, Cdouble,
                Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Cint),
               ctx(), polys, n, d, A, l, u, olo === nothing ? C_NULL : olo, ohi === nothing ? C_NULL : ohi, tol, slack_cap, opts,
               empty, how, eps, x, row, lam, iters, QPN_MEM_HOST)
    rc == 0 || error("qpn_exemplar_polys failed ($rc)")
    (empty, how, eps, x, row, lam, iters)
end

"""
    exemplar_products(A, l, u, piece_row, factors, n; open_lo=nothing, open_hi=nothing, point=nothing, point_of=nothing,
                      point_tol=1e-6, tol=1e-2, slack_cap=1.0, max_iters=0) -> (near, empty, how, eps, x, row, lambda, iters)

qpn_exemplar_products: the test of the intersection tree (src/intersection.jl:66-105) for products of pieces, one job per product.
The pieces are runs of rows of one pool: A [d, rows] (a pool row is a COLUMN of the Julia matrix, which is the row-major pool of the
ABI), l, u [rows], open_lo, open_hi [rows] (Bool or UInt8; nothing: closed), piece_row [pieces + 1] 0-based and ascending: piece p
(0-based) = the pool rows piece_row[p] .. piece_row[p + 1] - 1.  factors [k, products] Int32: the 0-based pieces of a product in slot
order, -1 = no factor in that slot; the rows of every product add up to n.  point [d, points] and point_of [products] (0-based), or
both nothing: the closure test l - point_tol <= a'p <= u + point_tol on every row; a product that fails it has near = 0, how = 6 and
row = the lowest 2 i + side violated, and no LP is solved for it.  The other outputs are those of exemplar_polys for the polyhedron
of the product's rows.  n <= 511, d <= 255, k <= 32.
"""
function exemplar_products(A::Matrix{Float64}, l::Vector{Float64}, u::Vector{Float64}, piece_row::Vector{Int32}, factors::Matrix{Int32},
                           n::Integer; open_lo::Union{Nothing,AbstractVector} = nothing, open_hi::Union{Nothing,AbstractVector} = nothing,
                           point::Union{Nothing,Matrix{Float64}} = nothing, point_of::Union{Nothing,Vector{Int32}} = nothing,
                           point_tol::Float64 = 1e-6, tol::Float64 = 1e-2, slack_cap::Float64 = 1.0, max_iters::Integer = 0)
    d, rows = size(A)
    k, products = size(factors)
    length(l) == rows && length(u) == rows && length(piece_row) >= 1 || error("exemplar_products: inconsistent shapes")
    (point === nothing) == (point_of === nothing) || error("exemplar_products: point and point_of go together")
    point === nothing || (size(point, 1) == d && length(point_of) == products) || error("exemplar_products: inconsistent shapes")
    flags(o) = o === nothing ? nothing : (length(o) == rows || error("exemplar_products: inconsistent shapes"); Vector{UInt8}(o .!= 0))
    olo = flags(open_lo); ohi = flags(open_hi)
    opts = Ref((1e-9, 1e-9, 1e-9, 1e-6, Int32(max_iters), Int32(0)))      # qpn_lp_opts
    near = zeros(UInt8, products); empty = zeros(UInt8, products); how = zeros(Int32, products); eps = zeros(products)
    x = zeros(d, products); row = zeros(Int32, products); lam = zeros(2n + 1, products); iters = zeros(Int32, products)
    rc = ccall((:qpn_exemplar_products, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Int32, Ptr{Int32}, Int32, Int32,
                Int32, Ptr{Int32}, Int32, Ptr{Cdouble}, Ptr{Int32}, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt8},
                Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Cint),
               ctx(), d, rows, A, l, u, olo === nothing ? C_NULL : olo, ohi === nothing ? C_NULL : ohi, length(piece_row) - 1, piece_row,
               products, n, k, factors, point === nothing ? 0 : size(point, 2), point === nothing ? C_NULL : point,
               point_of === nothing ? C_NULL : point_of, point_tol, tol, slack_cap, opts, near, empty, how, eps, x, row, lam, iters,
               QPN_MEM_HOST)
    rc == 0 || error("qpn_exemplar_products failed ($rc)")
    (near, empty, how, eps, x, row, lam, iters)
end

"""
    intersection_trees(A, l, u, piece_row, L, list_ptr, list_mem, list_red, cap; open_lo=nothing, open_hi=nothing, point=nothing,
                       point_of=nothing, point_tol=1e-6, tol=1e-2, slack_cap=1.0, max_iters=0)
        -> (leaves, leaf_tree, leaf_how, tree_leaves, tested, alive, unanswered, overflow)

qpn_intersection_trees: IntersectionRoot's walk (src/intersection.jl:66-105, :116-138) for `trees` trees of one depth L over the pool
of exemplar_products (A [d, rows], l, u, flags, piece_row 0-based), breadth first, the subtree under an empty prefix never formed.
list_ptr [trees L + 1] (0-based offsets) and list_mem (0-based pieces) are a CSR: list g L + t (0-based) holds the pieces of union t
of tree g in order, its last list_red[g L + t] members being complement pieces.  point [d, points] and point_of [trees] (0-based), or
both nothing.  cap: the most tuples a depth may hold.  leaves [L, n_leaves] (0-based pieces), leaf_tree and leaf_how [n_leaves], in
the order `iterate` yields them; tree_leaves [trees]; tested, alive, unanswered [L]; overflow: 0, or the depth that formed more
than cap candidates (no leaves then: ask again with a larger cap, or enumerate the products).  2 <= L <= 32, d <= 255, cap <= 2^22.
"""
function intersection_trees(A::Matrix{Float64}, l::Vector{Float64}, u::Vector{Float64}, piece_row::Vector{Int32}, L::Integer,
                            list_ptr::Vector{Int32}, list_mem::Vector{Int32}, list_red::Vector{Int32}, cap::Integer;
                            open_lo::Union{Nothing,AbstractVector} = nothing, open_hi::Union{Nothing,AbstractVector} = nothing,
                            point::Union{Nothing,Matrix{Float64}} = nothing, point_of::Union{Nothing,Vector{Int32}} = nothing,
                            point_tol::Float64 = 1e-6, tol::Float64 = 1e-2, slack_cap::Float64 = 1.0, max_iters::Integer = 0)
    d, rows = size(A)
    L >= 1 && length(list_red) % L == 0 && length(list_ptr) == length(list_red) + 1 || error("intersection_trees: inconsistent shapes")
    trees = length(list_red) ÷ L
    length(l) == rows && length(u) == rows && length(piece_row) >= 1 || error("intersection_trees: inconsistent shapes")
    (point === nothing) == (point_of === nothing) || error("intersection_trees: point and point_of go together")
    point === nothing || (size(point, 1) == d && length(point_of) == trees) || error("intersection_trees: inconsistent shapes")
    flags(o) = o === nothing ? nothing : (length(o) == rows || error("intersection_trees: inconsistent shapes"); Vector{UInt8}(o .!= 0))
    olo = flags(open_lo); ohi = flags(open_hi)
    opts = Ref((1e-9, 1e-9, 1e-9, 1e-6, Int32(max_iters), Int32(0)))      # qpn_lp_opts
    leaves = zeros(Int32, L, max(cap, 0)); leaf_tree = zeros(Int32, max(cap, 0)); leaf_how = zeros(Int32, max(cap, 0))
    n_leaves = zeros(Int64, 1); tree_leaves = zeros(Int32, trees)
    tested = zeros(Int64, L); alive = zeros(Int64, L); unanswered = zeros(Int64, L); overflow = zeros(Int32, 1)
    rc = ccall((:qpn_intersection_trees, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Int32, Ptr{Int32}, Int32, Int32,
                Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Cdouble}, Ptr{Int32}, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}, Int32,
                Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}, Cint),
               ctx(), d, rows, A, l, u, olo === nothing ? C_NULL : olo, ohi === nothing ? C_NULL : ohi, length(piece_row) - 1, piece_row,
               trees, L, length(list_mem), list_ptr, list_mem, list_red, point === nothing ? 0 : size(point, 2),
               point === nothing ? C_NULL : point, point_of === nothing ? C_NULL : point_of, point_tol, tol, slack_cap, opts, cap,
               leaves, leaf_tree, leaf_how, n_leaves, tree_leaves, tested, alive, unanswered, overflow, QPN_MEM_HOST)
    rc == 0 || error("qpn_intersection_trees failed ($rc)")
    k = Int(n_leaves[1])
    (leaves[:, 1:k], leaf_tree[1:k], leaf_how[1:k], tree_leaves, tested, alive, unanswered, Int(overflow[1]))
end

function verify_nodes(nodes::Nodes, xd::Matrix{Float64}, w::VecOrMat{Float64}; tol::Float64 = 1e-4)
    solution = zeros(Int32, nodes.batch); path = zeros(Int32, nodes.batch); lambda = zeros(max(nodes.m, 1), nodes.batch)
    rc = ccall((:qpn_verify_nodes_h, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Cint),
               ctx(), nodes.h, xd, w, ndims(w) == 1 ? Int64(0) : Int64(nodes.p), tol, solution, lambda, path, QPN_MEM_HOST)
    rc == 0 || error("qpn_verify_nodes_h failed ($rc)")
    (solution, lambda, path)
end

# The accept gate over the nodes `idx` names (1-based, any order, an entry may come more than once; qpn_verify_nodes_subset_h):
# column s of every array belongs to node idx[s] -- xd is n×count, w p×count (or a shared vector), the returned lambda m×count.
# Column s equals what verify_nodes returns for node idx[s] at the same xd and w columns, bit for bit; the launches cover count
# nodes, not the handle's batch.
function verify_nodes_subset(nodes::Nodes, idx::Vector{<:Integer}, xd::Matrix{Float64}, w::VecOrMat{Float64}; tol::Float64 = 1e-4)
    count = length(idx)
    size(xd) == (nodes.n, count) || error("verify_nodes_subset: xd must be n×count")
    ndims(w) == 1 || size(w, 2) == count || error("verify_nodes_subset: w must be p×count")
    all(i -> 1 <= i <= nodes.batch, idx) || error("verify_nodes_subset: idx entries must lie in 1:batch")
    idx0 = Int32.(idx .- 1)
    solution = zeros(Int32, count); path = zeros(Int32, count); lambda = zeros(max(nodes.m, 1), count)
    rc = ccall((:qpn_verify_nodes_subset_h, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Ptr{Int32}, Ptr{Cdouble},
                Ptr{Int32}, Cint),
               ctx(), nodes.h, Int32(count), idx0, xd, w, ndims(w) == 1 ? Int64(0) : Int64(nodes.p), tol, solution, lambda, path,
               QPN_MEM_HOST)
    rc == 0 || error("qpn_verify_nodes_subset_h failed ($rc)")
    (solution, lambda, path)
end

# ---- pool assembly (combine_gavis, src/avi.jl:305-377) and local pieces (local_piece, src/avi_solutions.jl:400-496) ----
struct PoolShape          # qpn_pool_shape, include/qpn_hip.h
    players::Int32
    nd::Int32
    p::Int32
    n_i::Ptr{Int32}
    m_i::Ptr{Int32}
    dpos::Ptr{Int32}
end
const QPN_POOL_REDUCED = Cint(0)
const QPN_POOL_REFERENCE = Cint(1)

"""
    (M, q, l, u, kind) = assemble_pool(n_i, m_i, dpos, nd, Qd, Qp, qd, Ad, Bp, lo, hi, w; form = QPN_POOL_REDUCED)

One Nash pool (the players' blocks stacked in pool order, see include/qpn_hip.h; `dpos` 0-based positions in dec_inds) as
the AVI `solve_avi_batch` takes: the device counterpart of `combine_gavis` (+ `convert` for `QPN_POOL_REFERENCE`).
"""
function assemble_pool(n_i::Vector{Int32}, m_i::Vector{Int32}, dpos::Vector{Int32}, nd::Integer, Qd::Matrix{Float64}, Qp::Matrix{Float64},
                       qd::Vector{Float64}, Ad::Matrix{Float64}, Bp::Matrix{Float64}, lo::Vector{Float64}, hi::Vector{Float64},
                       w::Vector{Float64}; form::Cint = QPN_POOL_REDUCED)
    GC.@preserve n_i m_i dpos begin
        shape = Ref(PoolShape(Int32(length(n_i)), Int32(nd), Int32(length(w)), pointer(n_i), pointer(m_i), pointer(dpos)))
        Nr = Ref{Int32}(0)
        ccall((:qpn_pool_size, LIB), Cint, (Ref{PoolShape}, Cint, Ref{Int32}), shape, form, Nr) == 0 || error("qpn_pool_size: bad shape")
        N = Int(Nr[])
        M = zeros(N, N); q = zeros(N); l = zeros(N); u = zeros(N); kind = zeros(UInt8, N)
        rc = ccall((:qpn_assemble_pools, LIB), Cint,
                   (Ptr{Cvoid}, Ref{PoolShape}, Cint, Int32, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64,
                    Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{UInt8}, Cint),
                   ctx(), shape, form, Int32(1), Qd, 0, Qp, 0, qd, 0, Ad, 0, Bp, 0, lo, hi, 0, w, 0, M, Int64(N * N), q, l, u, kind, QPN_MEM_HOST)
        rc == 0 || error("qpn_assemble_pools failed ($rc)")
        return (M, q, l, u, kind)
    end
end

"""
    (Ap, lp, up, keep) = local_pieces(Qd, R, qd, Ad, B, l, u, K)

`local_piece` (src/avi_solutions.jl:400-496, before `simplify`) for the recipes `K` ((n+m)×pieces UInt8 codes 1..8) of ONE
node's GAVI (process_solution_graph, src/avi.jl:447-477): `Ap` is 2(n+m) × (n+m+p) × pieces over [x_d; λ; x_p].
"""
function local_pieces(Qd::Matrix{Float64}, R::Matrix{Float64}, qd::Vector{Float64}, Ad::Matrix{Float64}, B::Matrix{Float64},
                      l::Vector{Float64}, u::Vector{Float64}, K::Matrix{UInt8})
    n = length(qd); m = length(l); p = size(R, 2); N = n + m; pieces = size(K, 2)
    Ap = zeros(2N, N + p, pieces); lp = zeros(2N, pieces); up = zeros(2N, pieces); keep = zeros(UInt8, 2N, pieces)
    node_of = zeros(Int32, pieces)
    rc = ccall((:qpn_local_pieces, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Cint),
               ctx(), Int32(pieces), Int32(1), Int32(n), Int32(m), Int32(p), Qd, R, qd, Ad, B, l, u, node_of, K, Ap, lp, up, keep, QPN_MEM_HOST)
    rc == 0 || error("qpn_local_pieces failed ($rc)")
    (Ap, lp, up, keep)
end

"""
    recipes_batch(masks, counts) -> (K, node_of)

`all_Ks` (src/avi_solutions.jl:200-215) for MANY solutions in one launch (`qpn_recipes_batch`): `masks` is N x nodes (the `active`
output of a solve, one column per node), `counts[b]` the number of recipes wanted of node b (at most the product of its rows'
code counts).  Returns the recipes K (N x total, one column per recipe) and the 0-based node of each.
"""
function recipes_batch(masks::Matrix{UInt8}, counts::Vector{<:Integer})
    N, nodes = size(masks)
    offsets = Int64[0; cumsum(Int64.(counts))]
    total = Int(offsets[end])
    K = zeros(UInt8, N, total); node_of = zeros(Int32, total)
    rc = ccall((:qpn_recipes_batch, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int32}, Cint),
               ctx(), Int32(nodes), Int32(N), masks, offsets, K, node_of, QPN_MEM_HOST)
    rc == 0 || error("qpn_recipes_batch failed ($rc)")
    (K, node_of)
end

"""
    recipes_batch_range(masks, first, counts) -> (K, node_of)

`recipes_batch` from a starting recipe per node (`qpn_recipes_batch_range`): node b gets the recipes `first[b] .. first[b] +
counts[b] - 1` (0-based) of its product, row 0 the fastest digit.  A range beyond the product is an error.
"""
function recipes_batch_range(masks::Matrix{UInt8}, first::Vector{<:Integer}, counts::Vector{<:Integer})
    N, nodes = size(masks)
    offsets = Int64[0; cumsum(Int64.(counts))]
    total = Int(offsets[end])
    K = zeros(UInt8, N, total); node_of = zeros(Int32, total)
    rc = ccall((:qpn_recipes_batch_range, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}, Ptr{Int64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int32}, Cint),
               ctx(), Int32(nodes), Int32(N), masks, Int64.(first), offsets, K, node_of, QPN_MEM_HOST)
    rc == 0 || error("qpn_recipes_batch_range failed ($rc)")
    (K, node_of)
end

"""
    finish_pieces(Ar, lr, ur, rows, flags, rec_of, ncols, take, xk, probe, n, m; member_tol = 1e-5)
        -> (status, worst, hash, dup_of, store_of, As, ls, us, rows_s)

The finishing step of `reduced_pieces`' output (`qpn_finish_pieces`): every piece over its item's columns `take[1:ncols[k], k]`
(0-based positions among the n + p columns, in ascending global order), normalised, with the point's worst violation, the merge
test, the 64-bit hash of the rounded key and the earliest equal earlier piece (`dup_of`, 0-based, -1: none).  `rec_of` is 0-based.
The store (`As[:, :, s]`, the cap x (n + p) row matrix of stored piece s) holds the members that are neither duplicates nor
flagged; `store_of[t]` is a piece's 0-based slot or -1.  Status bits: 1 member, 2 merge candidate, 4 duplicate, 8 flagged.
"""
function finish_pieces(Ar::Array{Float64,3}, lr::Matrix{Float64}, ur::Matrix{Float64}, rows::Vector{Int32}, flags::Vector{Int32},
                       rec_of::Vector{Int32}, ncols::Vector{Int32}, take::Matrix{Int32}, xk::Matrix{Float64}, probe::Matrix{Float64},
                       n::Integer, m::Integer; member_tol::Float64 = 1e-5)
    cap, oc, pieces = size(Ar); records = length(ncols); p = oc - n
    status = zeros(Int32, pieces); worst = zeros(pieces); hash = zeros(UInt64, pieces); dup_of = zeros(Int32, pieces)
    store_of = zeros(Int32, pieces)
    As = zeros(cap, oc, pieces); ls = zeros(cap, pieces); us = zeros(cap, pieces); rows_s = zeros(Int32, pieces)
    stored = Ref{Int32}(0)
    rc = ccall((:qpn_finish_pieces, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32},
                Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt64},
                Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ref{Int32}, Cint),
               ctx(), Int32(pieces), Int32(records), Int32(n), Int32(m), Int32(p), Ar, lr, ur, rows, flags, rec_of, ncols, take, xk,
               probe, member_tol, status, worst, hash, dup_of, store_of, Int32(pieces), As, ls, us, rows_s, stored, QPN_MEM_HOST)
    rc == 0 || error("qpn_finish_pieces failed ($rc)")
    S = Int(stored[])
    (status, worst, hash, dup_of, store_of, As[:, :, 1:S], ls[:, 1:S], us[:, 1:S], rows_s[1:S])
end

"""
    reduced_pieces(Qd, R, qd, Ad, B, l, u, K, node_of; tol = 1e-9) -> (Ar, lr, ur, rows, flags)

`local_piece` (src/avi_solutions.jl:400-496) for the recipes K (one column each) over the node records (third index = node, as
`solve_nodes!` takes them), with the m multiplier columns eliminated through each piece's own equality rows (`qpn_reduced_pieces`):
piece t lives on the records of node `node_of[t]` (0-based).  `Ar[:, :, t]` is the cap x (n + p) row matrix over `[x_d; x_p]`
(cap = n + 2m), of which the first `rows[t]` rows are live; `flags[t] != 0`: a multiplier was pinned by no equality row -- that
piece needs the polyhedral projection (src/avi_solutions.jl:79-91) on the host.
"""
function reduced_pieces(Qd::Array{Float64,3}, R::Array{Float64,3}, qd::Matrix{Float64}, Ad::Array{Float64,3}, B::Array{Float64,3},
                        l::Matrix{Float64}, u::Matrix{Float64}, K::Matrix{UInt8}, node_of::Vector{Int32}; tol::Float64 = 1e-9)
    n, nodes = size(qd); m = size(l, 1); p = size(R, 2); pieces = size(K, 2); cap = n + 2m
    Ar = zeros(cap, n + p, pieces); lr = zeros(cap, pieces); ur = zeros(cap, pieces)
    rows = zeros(Int32, pieces); flags = zeros(Int32, pieces)
    rc = ccall((:qpn_reduced_pieces, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Cint),
               ctx(), Int32(pieces), Int32(nodes), Int32(n), Int32(m), Int32(p), Qd, R, qd, Ad, B, l, u, node_of, K, tol, Ar, lr, ur, rows, flags,
               QPN_MEM_HOST)
    rc == 0 || error("qpn_reduced_pieces failed ($rc)")
    (Ar, lr, ur, rows, flags)
end

"""
    project_pieces(Qd, R, qd, Ad, B, l, u, K, node_of; tol = 1e-9, cap = min(4096, max(256, 4(n + 2m)))) -> (Ar, lr, ur, rows, flags)

`reduced_pieces` for the pieces it flags (`qpn_project_pieces`): after the elimination through a piece's own equality rows, every
multiplier column that no equality pins takes one Fourier-Motzkin step, in ascending order, all on the device.  `Ar[:, :, t]` is
the cap x (n + p) row matrix over `[x_d; x_p]` with `cap >= n + 2m` rows of room, of which the first `rows[t]` are live (redundant
rows are not removed).  `flags[t] == 4`: a step needed more than `cap` rows -- the piece comes back empty (`rows[t] == 0`); call
again with a larger `cap`.  `flags[t] == 2`: more than `cap` rows were alive before the first step.
"""
function project_pieces(Qd::Array{Float64,3}, R::Array{Float64,3}, qd::Matrix{Float64}, Ad::Array{Float64,3}, B::Array{Float64,3},
                        l::Matrix{Float64}, u::Matrix{Float64}, K::Matrix{UInt8}, node_of::Vector{Int32}; tol::Float64 = 1e-9,
                        cap::Integer = min(4096, max(256, 4 * (size(qd, 1) + 2 * size(l, 1)))))
    n, nodes = size(qd); m = size(l, 1); p = size(R, 2); pieces = size(K, 2)
    cap >= n + 2m || error("project_pieces: cap < n + 2m")
    Ar = zeros(cap, n + p, pieces); lr = zeros(cap, pieces); ur = zeros(cap, pieces)
    rows = zeros(Int32, pieces); flags = zeros(Int32, pieces)
    rc = ccall((:qpn_project_pieces, LIB), Cint,
               (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8}, Cdouble, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Cint),
               ctx(), Int32(pieces), Int32(nodes), Int32(n), Int32(m), Int32(p), Qd, R, qd, Ad, B, l, u, node_of, K, tol, Int32(cap), Ar, lr, ur,
               rows, flags, QPN_MEM_HOST)
    rc == 0 || error("qpn_project_pieces failed ($rc)")
    (Ar, lr, ur, rows, flags)
end

"""
    order_nodes_by_pivots!(pivots)

Schedule hint for later `solve_nodes!` calls over the same nodes (longest solves first); `pivots` is the
`pivots` output of an earlier sweep.  `clear_node_order!()` removes it.  Results do not depend on it.
"""
function order_nodes_by_pivots!(pivots::Vector{Int32})
    rc = ccall((:qpn_order_nodes_by_pivots, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Int32, Cint), ctx(), pivots, Int32(length(pivots)), QPN_MEM_HOST)
    rc == 0 || error("qpn_order_nodes_by_pivots failed ($rc)")
    nothing
end
# period (in calls) of the context's own refresh of that hint; 0 = off (default 16)
set_auto_schedule!(period::Integer) = (ccall((:qpn_ctx_set_auto_schedule, LIB), Cint, (Ptr{Cvoid}, Int32), ctx(), Int32(period)); nothing)
clear_node_order!() = (ccall((:qpn_set_node_order, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Int32, Cint), ctx(), C_NULL, Int32(0), QPN_MEM_HOST); nothing)
# kernel routes with identical contracts (A/B measurements; include/qpn_hip.h, QPN_OPT_*): MID_ROUTE 1 = fused workgroup kernel per
# node of 33 .. 128 variables or constraints (default; one wavefront per node up to 48), 0 = the general route (the cross-check);
# BIG_ROUTE takes 1 only (blocked crash straight from the records for nodes up to 256 x 256)
# SYM_ROUTE 1 = resident records whose Qd blocks are all bitwise symmetric take the kernel variants that use it (default), 0 = never.
const QPN_OPT_MID_ROUTE = Int32(1)
const QPN_OPT_BIG_ROUTE = Int32(2)
# CRASH_CACHE 1 = resident symmetric n = m = 32 records keep the part of the crash that Qd and Ad alone decide across sweeps
# (22 KB of HBM per node on top of the 22 KB of records; bit-identical results; default), 0 = never.
# LLC_BUDGET_MB: MiB of the last-level cache that sweeps over the crash cache count on -- a sweep whose records fit it while
# records + crash cache do not streams the crash cache (non-temporal loads) so that the records stay cached; 0 = never, -1 = always.
const QPN_OPT_SYM_ROUTE = Int32(3)
const QPN_OPT_CRASH_CACHE = Int32(4)
const QPN_OPT_LLC_BUDGET_MB = Int32(5)
# CRASH_CACHE_BIG 1 = resident records of the large class (64 < n <= 256, m <= 256: the blocked crash) keep what the elimination
# makes of Qd and Ad alone across sweeps (1.6 MB of HBM per node at n = m = 256 on top of 1.06 MB of records; bit-identical
# results, the same nodes decline), 0 = never (default).
const QPN_OPT_CRASH_CACHE_BIG = Int32(6)
# WARM_BIG 1 = sweeps with `warm =` over large resident nodes (64 < n <= 256, m <= 256) on the symmetric route start block principal
# pivoting from the set the hint's multipliers name (`pivots == n`: the hint held; results equal up to rounding), 0 = the hint is
# ignored in that class (default).
const QPN_OPT_WARM_BIG = Int32(7)
function set_option!(option::Integer, value::Integer)
    rc = ccall((:qpn_ctx_set_option, LIB), Cint, (Ptr{Cvoid}, Int32, Int32), ctx(), Int32(option), Int32(value))
    rc == 0 || error("qpn_ctx_set_option failed ($rc)")
    nothing
end

# ---- multi-GPU (one Julia process per GPU, e.g. under MPI.jl / Distributed): replicas of the iterate ----
# The ABI works on DEVICE pointers here (the host-array routes above stage through the library's workspace):
# `x_dev` below is an address inside a buffer from `shared_alloc`, e.g. wrapped by AMDGPU.jl's unsafe_wrap.
const QPN_IPC_HANDLE_BYTES = 64
const QPN_SHARED_FINE_GRAINED = Cint(1)
const QPN_SWEEP_BOX_BYTES = 512

"""
    shared_alloc(nbytes; fine_grained=false) -> (ptr::Ptr{Cvoid}, handle::Vector{UInt8})

Zeroed device buffer on this process's GPU and its IPC handle; send the handle to the peer processes
(MPI.Allgather, a socket, ...) and `shared_open` it there.
"""
function shared_alloc(nbytes::Integer; fine_grained::Bool = false)
    p = Ref{Ptr{Cvoid}}(C_NULL); h = zeros(UInt8, QPN_IPC_HANDLE_BYTES)
    rc = ccall((:qpn_shared_alloc, LIB), Cint, (Ptr{Cvoid}, Csize_t, Cint, Ref{Ptr{Cvoid}}, Ptr{UInt8}),
               ctx(), Csize_t(nbytes), fine_grained ? QPN_SHARED_FINE_GRAINED : Cint(0), p, h)
    rc == 0 || error("qpn_shared_alloc failed")
    (p[], h)
end
function shared_open(handle::Vector{UInt8})
    p = Ref{Ptr{Cvoid}}(C_NULL)
    ccall((:qpn_shared_open, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ref{Ptr{Cvoid}}), ctx(), handle, p) == 0 || error("qpn_shared_open failed")
    p[]
end
shared_close(p::Ptr{Cvoid}) = (ccall((:qpn_shared_close, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), p); nothing)
shared_free(p::Ptr{Cvoid}) = (ccall((:qpn_shared_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), p); nothing)

"""
    set_primal_mirrors!(own, nbytes, peers)

Later device-memory `qpn_solve_nodes_into` calls whose `x` lies inside `own` also store every primal block at the
same offset of each peer buffer (at most 7).  `set_primal_mirrors!()` clears.
"""
function set_primal_mirrors!(own::Ptr{Cvoid} = C_NULL, nbytes::Integer = 0, peers::Vector{Ptr{Cvoid}} = Ptr{Cvoid}[])
    rc = ccall((:qpn_set_primal_mirrors, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Int32, Ptr{Ptr{Cvoid}}),
               ctx(), own, Csize_t(nbytes), Int32(length(peers)), peers)
    rc == 0 || error("qpn_set_primal_mirrors failed")
    nothing
end

"""
    sweep_status!(out_dev, status_dev, resid_dev, count; rank=0, boxes=Ptr{Cvoid}[], epoch=0, timeout_ms=1000)

`out_dev[1:4]` (device) <- (items not solved, max resid, all ranks arrived, missed barriers so far), combined over
`length(boxes)` ranks through their mailboxes (each `QPN_SWEEP_BOX_BYTES`, `shared_alloc(...; fine_grained=true)`).
Asynchronous; enqueued after the solve it is also the barrier that completes the replicas (src/algorithm.jl:95-109).
"""
function sweep_status!(out_dev::Ptr{Cvoid}, status_dev::Ptr{Cvoid}, resid_dev::Ptr{Cvoid}, count::Integer;
                       rank::Integer = 0, boxes::Vector{Ptr{Cvoid}} = Ptr{Cvoid}[], epoch::Integer = 0, timeout_ms::Integer = 1000)
    world = max(length(boxes), 1)
    rc = ccall((:qpn_sweep_status, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int32, Ptr{Ptr{Cvoid}}, UInt64, Int32),
               ctx(), status_dev, resid_dev, Int32(count), out_dev, Int32(rank), Int32(world),
               world > 1 ? pointer(boxes) : Ptr{Ptr{Cvoid}}(C_NULL), UInt64(epoch), Int32(timeout_ms))
    rc == 0 || error("qpn_sweep_status failed")
    nothing
end

# A node record with its equality rows (l == u) moved into the free block: z = [x; mu_E; lambda_I].  The multiplier of an equality
# row is a free variable of the node's AVI (src/avi.jl:113-128), so this is the same complementarity system -- but the fused node
# kernels, which decline a record that carries an equality row, take it (DESIGN.md section 5a; the Python mirror's
# level_batch.free_equalities).  Every parent's record has such rows: its children's pieces.  Arrays in MATH layout (row-major
# meaning: Qd n x n, R n x p, Ad m x n, B m x p); returns the rewritten record and nx = n (the first nx entries of z are x).
function free_equalities(Qd::AbstractMatrix, R::AbstractMatrix, qd::AbstractVector, Ad::AbstractMatrix, B::AbstractMatrix,
                         l::AbstractVector, u::AbstractVector)
    E = findall(i -> isfinite(l[i]) && l[i] == u[i], eachindex(l))
    isempty(E) && return (Qd, R, qd, Ad, B, l, u, size(Qd, 1))
    I = setdiff(collect(eachindex(l)), E)
    ne = length(E)
    Qd2 = [Qd -transpose(Ad[E, :]); Ad[E, :] zeros(ne, ne)]
    R2 = [R; B[E, :]]
    qd2 = [qd; -l[E]]
    Ad2 = [Ad[I, :] zeros(length(I), ne)]
    return (Qd2, R2, qd2, Ad2, B[I, :], l[I], u[I], size(Qd, 1))
end

# ---- drop-in bodies -------------------------------------------------------------------------------
# src/avi.jl:63-77 with the PATH call replaced; StatusCode / check_avi_solution stay the reference's.
function solve_avi_hip(QPN, avi, z0, w; convergence_tolerance = 1e-10)
    (st, z, info) = solve_mcp(avi.M, avi.N * w + avi.o, avi.l, avi.u, collect(Float64, z0))
    (; sol_bad, degree, r) = QPN.check_avi_solution(avi, z, w)          # kept: src/avi.jl:71
    sol_bad && return (; z, status = QPN.FAILURE, info = (; path_status = st, info))
    status = st == QPN_SUCCESS ? QPN.SUCCESS : QPN.FAILURE
    (; z, status, info = (; path_status = st, info))
end

# src/qp_processing.jl:12-33 (PATH branch): same MCP, same error convention (:30).
function solve_qp_hip(Q, q, A, l, u)
    n = size(Q, 1); m = size(A, 1)
    M = SparseMatrixCSC{Float64,Int32}([Q -A' spzeros(n, m); A spzeros(m, m) -sparse(1.0I, m, m); spzeros(m, n) sparse(1.0I, m, m) spzeros(m, m)])
    (st, z, _) = solve_mcp(M, [q; zeros(2m)], [fill(-Inf, n + m); l], [fill(Inf, n + m); u], zeros(2m + n))
    st == QPN_SUCCESS || error("Solver failure. Status value is $st")
    z[1:n]
end

"""
Overrides `solve_avi` (src/avi.jl:63-77) of the loaded QuadraticProgramNetworks module.  The PATH
branch of `solve_qp` (src/qp_processing.jl:12-33) shares its function with the OSQP branch, so it is
rerouted by the three-line source edit shown in INTEGRATION.md (calls `QPNHip.solve_qp_hip`).
"""
function install!(QPN = Main.QuadraticProgramNetworks)
    @eval QPN solve_avi(avi::AVI, z0, w; convergence_tolerance = 1e-10) = $(solve_avi_hip)($QPN, avi, z0, w; convergence_tolerance)
    nothing
end

end # module
