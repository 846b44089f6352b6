# TFHEMI355X.jl — puts libtfhe_mi355x.so behind TFHE.jl's OWN gate functions.
#
# NOT EXECUTED IN THE BUILD IMAGE (no Julia there): kept literal so it can be reviewed by reading against
# include/tfhe_mi355x.h; tests/test_julia_shim.py checks every ccall against the header, that no TFHE name is exported
# without being imported from TFHE, that every exported gate has its batched `broadcasted` method, and every size(...)
# destructuring against the reference's comprehension order.  One command runs it where Julia exists (INTEGRATION.md §2):
#     julia --project=julia/TFHEMI355X -e 'using Pkg; Pkg.develop(path="<TFHE.jl checkout>"); Pkg.test()'
#
# The module defines NO function named gate_*: it `import`s TFHE's functions (src/TFHE.jl:34-46,61) and adds methods
# whose cloud-key argument is a GpuCloudKey / GpuMKCloudKey.  After
#
#     using TFHE, Random
#     using TFHEMI355X                                        # the package julia/TFHEMI355X (Project.toml: deps TFHE, Random); exports only GpuCloudKey, GpuMKCloudKey, GpuLweArray, ...
#     rng = MersenneTwister(123)
#     secret_key, cloud_key = make_key_pair(rng)
#     gck = GpuCloudKey(cloud_key)                            # flattens + uploads the keys once (device 0)
#
# the reference's caller lines run unchanged with `gck` where they say `cloud_key`:
#
#     cresult = gate_xor.(gck, ciphertext1, ciphertext2)      # docs/src/manual.md:35 — ONE tfhe_gates_batch call
#     tmp = gate_xnor(gck, a, b); gate_mux(gck, tmp, lsb_carry, a)          # examples/tutorial.jl:44-45
#     tmps1 = gate_constant(gck, false)                       # examples/tutorial.jl:54
#     [gate_mux(gck, tmps1, b[i], a[i]) for i in 1:nb_bits]   # examples/tutorial.jl:62 (or gate_mux.(gck, tmps1, b, a): one call)
#     enc_out = mk_gate_nand(mck, enc_mess1, enc_mess2)       # test/runtests.jl:95, mck = GpuMKCloudKey(cloud_key)
#
# (examples/tutorial.jl annotates its own helper functions `ck::CloudKey`; to pass a GpuCloudKey through them the
# annotation has to be dropped or widened — CloudKey is a concrete struct, nothing can subtype it.)
#
#     gck8 = GpuCloudKey(cloud_key; devices=0:7)              # keys replicated on 8 GPUs, every batch call split over them
#     d1 = upload(gck, ciphertext1); d2 = upload(gck, ciphertext2)          # GpuLweArray: ciphertexts resident on the GPU
#     d3 = gate_and.(gck, gate_xor.(gck, d1, d2), d1)         # stays on the device between gates (tfhe_gates_level)
#     result = download(d3)                                   # Vector{LweSample}
module TFHEMI355X

using TFHE
import TFHE: gate_nand, gate_or, gate_and, gate_xor, gate_xnor, gate_not, gate_constant,
             gate_nor, gate_andny, gate_andyn, gate_orny, gate_oryn, gate_mux, mk_gate_nand
using TFHE: LweSample, LweParams, CloudKey, SecretKey, SchemeParameters, MKCloudKey, MKLweSample
using Random: AbstractRNG, RandomDevice
import Base.Broadcast: broadcastable, broadcasted

export GpuCloudKey, GpuMKCloudKey, GpuLweArray, gates_batch, gates_batch_async, PendingGates, upload, download, tgsw_load!, extern_mul, cmux_tree, cmux_net, rot_net, blind_rotate, mk_tgsw_load!, mk_extern_mul, mk_cmux_tree, mk_cmux_net, mk_rot_net, mk_blind_rotate, tlwe_alloc!, tlwe_upload!, tlwe_download, tgsw_update!, rot_net_level!, blind_rotate_level!, mk_tlwe_alloc!, mk_tlwe_upload!, mk_tlwe_download, mk_tgsw_update!, mk_tgsw_expand_update!, mk_rot_net_level!, mk_blind_rotate_level!, bootstrap_acc, bootstrap_acc_level!, mk_bootstrap_acc, mk_bootstrap_acc_level!

# the shared library as this repository builds it (make -C tfhe.jl_amd/csrc), or wherever TFHE_MI355X_LIB points
const LIB = get(ENV, "TFHE_MI355X_LIB", joinpath(@__DIR__, "..", "..", "..", "tfhe.jl_amd", "lib", "libtfhe_mi355x.so"))

# ABI check at load time (include/tfhe_mi355x.h: TFHE_MI355X_ABI_VERSION).  A NEGATIVE answer is a development build of the
# library (-DTFHE_EXPERIMENT, csrc/experiment.hpp: in-kernel stamps, environment-variable overrides): refused unless the user
# asked for it.
const ABI_VERSION = Int32(7)
function __init__()
    v = ccall((:tfhe_abi_version, LIB), Int32, ())
    if v < 0 && get(ENV, "TFHE_MI355X_ALLOW_EXPERIMENT", "") == ""
        error("$LIB is a development build (ABI version $v): set TFHE_MI355X_ALLOW_EXPERIMENT=1 to load it knowingly")
    end
    abs(v) == ABI_VERSION || error("$LIB has ABI version $v, this package needs $ABI_VERSION: rebuild it (make -C tfhe.jl_amd/csrc)")
end

# include/tfhe_mi355x.h: struct tfhe_params
struct TfheParams
    n::Int32; N::Int32; k::Int32; bs_l::Int32; bs_log2_base::Int32
    ks_t::Int32; ks_log2_base::Int32; parties::Int32
end

TfheParams(p::SchemeParameters) = TfheParams(
    p.lwe_size, p.tlwe_polynomial_degree, p.tlwe_mask_size, p.bs_decomp_length,
    p.bs_log2_base, p.ks_decomp_length, p.ks_log2_base, p.max_parties)

# opcodes (include/tfhe_mi355x.h: TFHE_GATE_*)
const NAND, OR, AND, XOR, XNOR, NOT, NOR, ANDNY, ANDYN, ORNY, ORYN, MUX, CONST0, CONST1, COPY =
    UInt8.(0:14)

function check(ctx::Ptr{Cvoid}, rc::Int32)
    rc == 0 && return
    msg = unsafe_string(ccall((:tfhe_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))
    error("tfhe_mi355x error $rc: $msg")
end

# One caller at a time per context (include/tfhe_mi355x.h, "Threading"): the library answers an overlapping call from another
# thread with TFHE_ERR_STATE; Julia tasks sharing a key therefore take the context's lock around every call (re-entrant: the
# scalar gate methods call the batch methods).  The lock also covers tfhe_last_error, whose message belongs to the owner.
const CTX_LOCKS = Dict{Ptr{Cvoid}, ReentrantLock}()
const CTX_LOCKS_GUARD = ReentrantLock()
ctx_lock(ctx::Ptr{Cvoid}) = lock(CTX_LOCKS_GUARD) do
    get!(() -> ReentrantLock(), CTX_LOCKS, ctx)
end
macro locked(ctx, ex)
    quote
        local lk = ctx_lock($(esc(ctx)))
        lock(lk)
        try
            $(esc(ex))
        finally
            unlock(lk)
        end
    end
end

# tfhe_ctx_create (one device) or tfhe_ctx_create_multi (keys replicated, batch calls fanned out inside the library)
function create_context(p::SchemeParameters, devices)
    tp = TfheParams(p)
    ctxref = Ref{Ptr{Cvoid}}(C_NULL)
    ids = Int32.(collect(devices))
    rc = if length(ids) == 1
        ccall((:tfhe_ctx_create, LIB), Int32, (Ref{TfheParams}, Int32, Ref{Ptr{Cvoid}}), tp, ids[1], ctxref)
    else
        ccall((:tfhe_ctx_create_multi, LIB), Int32, (Ref{TfheParams}, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
              tp, ids, Int32(length(ids)), ctxref)
    end
    check(Ptr{Cvoid}(C_NULL), rc)
    warn_if_inexact(ctxref[], p)
    ctxref[]
end

# tfhe_get_option "exact_domain" (ABI v7): 0 = the parameter set is outside what a Float64 transform computes exactly — the
# reference warns about the same limit (src/polynomials.jl:135-144); said once per parameter set
const WARNED_INEXACT = Set{Any}()
function warn_if_inexact(ctx::Ptr{Cvoid}, p::SchemeParameters)
    opt(name) = (v = Ref{Int64}(0); ccall((:tfhe_get_option, LIB), Int32, (Ptr{Cvoid}, Cstring, Ref{Int64}), ctx, name, v) == 0 ? v[] : Int64(-1))
    opt("exact_domain") == 0 || return
    key = (p.tlwe_polynomial_degree, p.tlwe_mask_size, p.bs_decomp_length, p.bs_log2_base, p.max_parties)
    key in WARNED_INEXACT && return
    push!(WARNED_INEXACT, key)
    @warn "TFHE parameter set is outside the Float64 exactness domain: result words may differ from the exact negacyclic product" predicted_rounding_margin = opt("exact_margin_x1e6") / 1e6 log2_worst_case_magnitude = opt("exact_bound_log2_x1000") / 1e3
end

# KeyswitchKey: key[h, j, i]::LweSample (src/keyswitch.jl:12,35-38) -> Int32 [kN][t][base-1][n+1] (C order)
function flatten_keyswitch_key(ks, n)
    base1, t, kN = size(ks.key)
    flat = Array{Int32}(undef, n + 1, base1, t, kN)                   # column-major: n+1 fastest
    for i in 1:kN, j in 1:t, h in 1:base1
        s = ks.key[h, j, i]
        flat[1:n, h, j, i] .= s.a
        flat[n + 1, h, j, i] = s.b
    end
    flat
end

# BootstrapKey: only the transformed form exists (src/bootstrap.jl:12-14).  Flatten
# key[i].samples[p, j].a[c].coeffs (Complex{Float64}[N/2]) to C order [n][l][k+1][k+1][N/2].
function flatten_bootstrap_spectra(bk, p::SchemeParameters)
    n, l, k1, M = p.lwe_size, p.bs_decomp_length, p.tlwe_mask_size + 1, p.tlwe_polynomial_degree ÷ 2
    spectra = Array{Complex{Float64}}(undef, M, k1, k1, l, n)        # column-major: M fastest
    for i in 1:n, pp in 1:l, j in 1:k1, c in 1:k1
        spectra[:, c, j, pp, i] .= bk.key[i].samples[pp, j].a[c].coeffs
    end
    spectra
end

"""
    GpuCloudKey(ck::CloudKey; device=0, devices=nothing, wires=65536)
    GpuCloudKey(rng, secret_key::SecretKey; device=0, devices=nothing, wires=65536)

A `CloudKey` resident on one MI355X (`device`) or replicated on several (`devices=0:7`).  Pass it to TFHE's own
`gate_*` functions in place of the `CloudKey`.  `wires` is the capacity (in ciphertexts) of the device-resident table
behind [`GpuLweArray`](@ref); it is allocated on first use.
"""
mutable struct GpuCloudKey
    params::SchemeParameters
    ctx::Ptr{Cvoid}
    # device-resident ciphertexts (tfhe_wires_*): rows of one table, handed out here, handed back by GpuLweArray finalizers
    wire_capacity::Int
    wire_ready::Bool                       # tfhe_wires_alloc done
    wire_next::Int
    wire_free::Vector{Int32}
    wire_returned::Vector{Vector{Int32}}

    # the finalizer is attached before anything that can throw: a failed key load does not leak the context
    function GpuCloudKey(p::SchemeParameters, devices, wires::Integer)
        ctx = create_context(p, devices)
        gck = new(p, ctx, Int(wires), false, 0, Int32[], Vector{Vector{Int32}}())
        finalizer(destroy!, gck)
        # no per-phase timing events: nothing in this module reads them, and every record keeps the stream's next kernel
        # waiting ~5 us (six per circuit level; include/tfhe_mi355x.h, tfhe_set_option)
        @locked ctx check(ctx, ccall((:tfhe_set_option, LIB), Int32, (Ptr{Cvoid}, Cstring, Int64), ctx, "timing_events", Int64(0)))
        gck
    end
end

function destroy!(g)
    if g.ctx != C_NULL
        ccall((:tfhe_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), g.ctx)    # (its entry in CTX_LOCKS stays: this may run as a finalizer, which must not take locks; a reused address finds a valid lock)
        g.ctx = C_NULL
    end
    nothing
end

function GpuCloudKey(ck::CloudKey; device::Integer=0, devices=nothing, wires::Integer=65536)
    p = ck.params
    gck = GpuCloudKey(p, devices === nothing ? [device] : devices, wires)
    try
        spectra = flatten_bootstrap_spectra(ck.bootstrap_key, p)
        GC.@preserve spectra @locked gck.ctx check(gck.ctx, ccall((:tfhe_load_bootstrap_key_c128, LIB), Int32,
            (Ptr{Cvoid}, Ptr{Complex{Float64}}), gck.ctx, spectra))
        flat = flatten_keyswitch_key(ck.keyswitch_key, p.lwe_size)
        GC.@preserve flat @locked gck.ctx check(gck.ctx, ccall((:tfhe_load_keyswitch_key, LIB), Int32,
            (Ptr{Cvoid}, Ptr{Int32}), gck.ctx, flat))
    catch
        destroy!(gck)
        rethrow()
    end
    gck
end

# The cloud key generated ON THE GPU (tfhe_keygen_cloud_key) instead of by CloudKey(rng, secret_key) on the host
# (api.jl:111-127): the TLWE key bits and a seed of six 32-bit words come from `rng` (for real keys: a cryptographic
# generator such as RandomDevice()), the bootstrap and keyswitch keys never exist on the host.  The key material follows
# the library's Philox streams, not MersenneTwister's.  Four of the seed words key the noise and are as secret as the
# secret key (they regenerate the noise of every key row): the seed is not stored anywhere.
function GpuCloudKey(rng::AbstractRNG, secret_key::SecretKey; device::Integer=0, devices=nothing, wires::Integer=65536,
                     noise_seed=nothing)     # (tests only: four fixed words instead of RandomDevice())
    p = secret_key.params
    gck = GpuCloudKey(p, devices === nothing ? [device] : devices, wires)
    try
        lwe_bits = Int32.(secret_key.key.key)                                        # lwe.jl:11-17
        tlwe_bits = Int32.(rand(rng, Bool, p.tlwe_polynomial_degree, p.tlwe_mask_size))   # [N, k] = C-order [k][N]; tlwe.jl:15-20
        # words 1-2 key the public masks (from `rng`: reproducible), words 3-6 (128 bits) key the noise: secret, drawn from the
        # operating system's generator whatever `rng` is (Philox then only expands that secret), discarded here
        seed = vcat(rand(rng, UInt32, 2), noise_seed === nothing ? rand(RandomDevice(), UInt32, 4) : UInt32.(noise_seed))
        length(seed) == 6 || error("GpuCloudKey: noise_seed must be four 32-bit words")
        GC.@preserve lwe_bits tlwe_bits seed @locked gck.ctx check(gck.ctx, ccall((:tfhe_keygen_cloud_key, LIB), Int32,
            (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Float64, Float64, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}),
            gck.ctx, lwe_bits, tlwe_bits, p.bs_noise_stddev, p.ks_noise_stddev, seed, C_NULL, C_NULL))
    catch
        destroy!(gck)
        rethrow()
    end
    gck
end

# a GpuCloudKey is a scalar under broadcasting, as CloudKey is (src/api.jl:130)
broadcastable(g::GpuCloudKey) = Ref(g)

# LweSample <-> flat Int32[n+1] (a then b), include/tfhe_mi355x.h
function flatten(xs::AbstractVector{LweSample})
    n = xs[1].params.size
    m = Array{Int32}(undef, n + 1, length(xs))
    for (g, x) in enumerate(xs)
        m[1:n, g] .= x.a
        m[n + 1, g] = x.b
    end
    m
end

unflatten(m::Matrix{Int32}, params::LweParams) =
    # current_variance is write-only bookkeeping in the reference (SURVEY §5); 0.0 as tlwe.jl:58 does
    [LweSample(params, m[1:end-1, g], m[end, g], 0.) for g in 1:size(m, 2)]

# ---- device-resident ciphertexts ------------------------------------------------------------------------------------
"""
    GpuLweArray

A vector of LWE samples resident on the GPU (rows of the key's wire table, tfhe_wires_*).  `upload(gck, xs)` makes
one, `download(d)` brings it back as `Vector{LweSample}`; gates on GpuLweArrays run through `tfhe_gates_level` and
return GpuLweArrays, so a circuit's intermediate ciphertexts never cross PCIe and are never re-flattened.
"""
mutable struct GpuLweArray
    key::GpuCloudKey
    rows::Vector{Int32}            # wire indices (0-based)

    function GpuLweArray(key::GpuCloudKey, rows::Vector{Int32})
        d = new(key, rows)
        # a finalizer must not call into the allocator: it only queues the rows; alloc_rows! takes them back
        finalizer(a -> push!(a.key.wire_returned, a.rows), d)
        d
    end
end

Base.length(d::GpuLweArray) = length(d.rows)

function alloc_rows!(g::GpuCloudKey, count::Int)
    if !g.wire_ready                                                       # first use: allocate the table
        @locked g.ctx check(g.ctx, ccall((:tfhe_wires_alloc, LIB), Int32, (Ptr{Cvoid}, Int64), g.ctx, g.wire_capacity))
        g.wire_ready = true
    end
    returned = g.wire_returned
    g.wire_returned = Vector{Vector{Int32}}()
    for r in returned
        append!(g.wire_free, r)
    end
    rows = Vector{Int32}(undef, count)
    reused = min(count, length(g.wire_free))
    for i in 1:reused
        rows[i] = pop!(g.wire_free)
    end
    fresh = count - reused
    if g.wire_next + fresh > g.wire_capacity
        append!(g.wire_free, rows[1:reused])
        error("GpuLweArray: wire table full ($(g.wire_capacity) ciphertexts); construct the GpuCloudKey with a larger `wires`")
    end
    for i in 1:fresh
        rows[reused + i] = g.wire_next + i - 1
    end
    g.wire_next += fresh
    rows
end

"""
    upload(gck, xs::AbstractVector{LweSample}) -> GpuLweArray
"""
function upload(g::GpuCloudKey, xs::AbstractVector{LweSample})
    rows = alloc_rows!(g, length(xs))
    isempty(xs) && return GpuLweArray(g, rows)
    flat = flatten(xs)
    first_fresh = isempty(rows) ? 0 : rows[1]
    contiguous = rows == collect(Int32, first_fresh:(first_fresh + length(rows) - 1))
    if contiguous
        GC.@preserve flat @locked g.ctx check(g.ctx, ccall((:tfhe_wires_upload, LIB), Int32,
            (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}), g.ctx, first_fresh, length(rows), flat))
    else                                                                 # recycled rows: one copy per row
        n1 = size(flat, 1)
        for (i, r) in enumerate(rows)
            GC.@preserve flat @locked g.ctx check(g.ctx, ccall((:tfhe_wires_upload, LIB), Int32,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}), g.ctx, r, 1, pointer(flat, (i - 1) * n1 + 1)))
        end
    end
    GpuLweArray(g, rows)
end

"""
    download(d::GpuLweArray) -> Vector{LweSample}
"""
function download(d::GpuLweArray)
    g = d.key
    out = Array{Int32}(undef, g.params.lwe_size + 1, length(d))
    GC.@preserve out @locked g.ctx check(g.ctx, ccall((:tfhe_wires_gather, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}), g.ctx, d.rows, length(d), out))
    unflatten(out, LweParams(g.params.lwe_size))
end

# ---- the batch calls ------------------------------------------------------------------------------------------------
const LweVec = AbstractVector{LweSample}
const LweOperand = Union{LweSample, LweVec, GpuLweArray}

operand_length(x::LweSample) = 1
operand_length(x) = length(x)

# the common length of the vector operands (scalars repeat, as under broadcasting)
function batch_length(operands)
    B = 1
    for x in operands
        x isa LweSample && continue
        L = operand_length(x)
        (B == 1 || L == B || L == 1) || throw(DimensionMismatch("gate operands of lengths $B and $L"))
        B = max(B, L)
    end
    B
end

expand(x::LweSample, B) = fill(x, B)
expand(xs::LweVec, B) = length(xs) == B ? xs : fill(xs[1], B)

"""
    gates_batch(gck, opcodes, xs, ys=nothing, zs=nothing)

`length(opcodes)` independent gates, one opcode per gate, in one GPU call (tfhe_gates_batch).
"""
function gates_batch(gck::GpuCloudKey, opcodes::Vector{UInt8}, xs, ys=nothing, zs=nothing)
    B = length(opcodes)
    params = LweParams(gck.params.lwe_size)
    B == 0 && return LweSample[]
    fx = xs === nothing ? nothing : flatten(xs)
    fy = ys === nothing ? nothing : flatten(ys)
    fz = zs === nothing ? nothing : flatten(zs)
    out = Array{Int32}(undef, gck.params.lwe_size + 1, B)
    ptr(a) = a === nothing ? Ptr{Int32}(C_NULL) : pointer(a)
    GC.@preserve fx fy fz out opcodes @locked gck.ctx check(gck.ctx, ccall((:tfhe_gates_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64),
        gck.ctx, opcodes, ptr(fx), ptr(fy), ptr(fz), out, B))
    unflatten(out, params)
end

"""
    bootstrap_tv(gck, tables, xs, index=nothing; with_keyswitch=true)  ->  Vector{LweSample}

Programmable bootstrapping (tfhe_bootstrap_tv_batch): `blind_rotate_and_extract(v, bk, barb, bara)` (bootstrap.jl:50-59) of every
sample with the test polynomial `v = tables[:, index[g]]` (`tables`: Int32 N x n_tv, one table per column; `index`: 1-based, or
`nothing` for the first table) instead of `repeat([mu], N)`, keyswitched (bootstrap.jl:92-95) unless `with_keyswitch = false`
(then the extracted samples of size k N).
"""
function bootstrap_tv(gck::GpuCloudKey, tables::AbstractMatrix{Int32}, xs, index=nothing; with_keyswitch::Bool=true)
    B = length(xs)
    B == 0 && return LweSample[]
    N = gck.params.tlwe_polynomial_degree
    size(tables, 1) == N || error("tfhe_mi355x: test polynomials must have N = ", N, " rows")
    tv = Matrix{Int32}(tables)
    idx = index === nothing ? nothing : Int32.(collect(index) .- 1)
    fx = flatten(xs)
    n_out = with_keyswitch ? gck.params.lwe_size : gck.params.tlwe_mask_size * N
    out = Array{Int32}(undef, n_out + 1, B)
    GC.@preserve tv idx fx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_bootstrap_tv_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Int32),
        gck.ctx, tv, Int32(size(tv, 2)), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), fx, out, B, Int32(with_keyswitch)))
    unflatten(out, LweParams(n_out))
end

"""
    bootstrap_tv_multi(gck, tables, xs, n_out, index=nothing; with_keyswitch=true)  ->  Vector{Vector{LweSample}}

Multi-output programmable bootstrapping (tfhe_bootstrap_tv_multi_batch): `bootstrap_tv` returning `n_out` results per sample from one
blind rotation, result `j` (1-based) the sample extracted at the accumulator's coefficient `(j - 1) N / n_out` instead of 0
(tlwe.jl:55-59).  With a table packing `f_j(m)` at window `(j - 1) p + m` of Z_{p n_out} and inputs encrypted in Z_{p n_out}, result
`j` encrypts `f_j(m)`.  `n_out`: a power of two <= 32, and 1 or <= N / 4.  Returns `n_out` vectors of `length(xs)` samples.
"""
function bootstrap_tv_multi(gck::GpuCloudKey, tables::AbstractMatrix{Int32}, xs, n_out::Integer, index=nothing; with_keyswitch::Bool=true)
    B = length(xs)
    B == 0 && return [LweSample[] for _ in 1:max(n_out, 0)]
    N = gck.params.tlwe_polynomial_degree
    size(tables, 1) == N || error("tfhe_mi355x: test polynomials must have N = ", N, " rows")
    1 <= n_out <= 32 || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32)")
    tv = Matrix{Int32}(tables)
    idx = index === nothing ? nothing : Int32.(collect(index) .- 1)
    fx = flatten(xs)
    width = with_keyswitch ? gck.params.lwe_size : gck.params.tlwe_mask_size * N
    out = Array{Int32}(undef, width + 1, n_out, B)
    GC.@preserve tv idx fx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_bootstrap_tv_multi_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int64, Int32),
        gck.ctx, tv, Int32(size(tv, 2)), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), Int32(n_out), fx, out, B, Int32(with_keyswitch)))
    [unflatten(out[:, j, :], LweParams(width)) for j in 1:n_out]
end

"""
    bootstrap_tv(gck, tables, d::GpuLweArray, index=nothing)              ->  GpuLweArray
    bootstrap_tv_multi(gck, tables, d::GpuLweArray, n_out, index=nothing)  ->  Vector{GpuLweArray}

`bootstrap_tv` / `bootstrap_tv_multi` on device-resident samples (tfhe_lut_level with one term of coefficient 1 per row): the results
are new rows of the wire table, keyswitched, so a chain of LUTs never crosses PCIe.  Asynchronous as the gates on GpuLweArrays.
"""
function lut_on_device(g::GpuCloudKey, tables::AbstractMatrix{Int32}, d::GpuLweArray, n_out::Integer, index)
    d.key === g || error("GpuLweArray belongs to another GpuCloudKey")
    B = length(d)
    N = g.params.tlwe_polynomial_degree
    size(tables, 1) == N || error("tfhe_mi355x: test polynomials must have N = ", N, " rows")
    1 <= n_out <= 32 || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32)")
    B == 0 && return Int32[]
    tv = Matrix{Int32}(tables)
    idx = index === nothing ? nothing : Int32.(collect(index) .- 1)
    term_start = collect(Int32, 0:B)
    coef = ones(Int32, B)
    out = alloc_rows!(g, B * n_out)
    GC.@preserve tv idx term_start coef out d @locked g.ctx check(g.ctx, ccall((:tfhe_lut_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64),
        g.ctx, tv, Int32(size(tv, 2)), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), Int32(n_out), term_start, d.rows, coef,
        Ptr{Int32}(C_NULL), out, B))
    out
end

bootstrap_tv(g::GpuCloudKey, tables::AbstractMatrix{Int32}, d::GpuLweArray, index=nothing) =
    GpuLweArray(g, lut_on_device(g, tables, d, 1, index))

function bootstrap_tv_multi(g::GpuCloudKey, tables::AbstractMatrix{Int32}, d::GpuLweArray, n_out::Integer, index=nothing)
    out = lut_on_device(g, tables, d, n_out, index)          # row g's output j is out[(g - 1) n_out + j]
    [GpuLweArray(g, out[j:n_out:end]) for j in 1:n_out]
end

"""
    tgsw_load!(gck, tgsw::Array{Int32})

The selector set of `extern_mul` / `cmux_tree` (tfhe_tgsw_load): `forward_transform(::TGswSample)` (tgsw.jl:120-121) of `S` TGSW
samples given as Int32 `N x (k+1) x (k+1) x l x S` (column-major: the C layout [S][l][k+1][k+1][N], `samples[p, j].a[c]` of
tgsw.jl:25-32).  Replaces any earlier set.
"""
function tgsw_load!(gck::GpuCloudKey, tgsw::Array{Int32})
    p = gck.params
    per = p.tlwe_polynomial_degree * (p.tlwe_mask_size + 1)^2 * p.bs_decomp_length
    (length(tgsw) > 0 && length(tgsw) % per == 0) || error("tfhe_mi355x: TGSW samples must hold a positive multiple of ", per, " words")
    GC.@preserve tgsw @locked gck.ctx check(gck.ctx, ccall((:tfhe_tgsw_load, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64), gck.ctx, tgsw, Int64(length(tgsw) ÷ per)))
    gck
end

"""
    extern_mul(gck, tlwe::Array{Int32,3}, sel)  ->  Array{Int32,3}

`tgsw_extern_mul(accum, gsw)` (tgsw.jl:125-129) for a batch (tfhe_extern_mul_batch): sample `g` of `tlwe` (Int32 `N x (k+1) x B`) times
loaded selector `sel[g]` (1-based).
"""
function extern_mul(gck::GpuCloudKey, tlwe::Array{Int32,3}, sel)
    p = gck.params
    size(tlwe)[1:2] == (p.tlwe_polynomial_degree, p.tlwe_mask_size + 1) || error("tfhe_mi355x: TLWE samples must be N x (k+1) x B")
    B = size(tlwe, 3)
    idx = Int32.(collect(sel) .- 1)
    length(idx) == B || error("tfhe_mi355x: one selector per sample")
    out = similar(tlwe)
    B == 0 && return out
    GC.@preserve tlwe idx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_extern_mul_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64), gck.ctx, tlwe, idx, out, Int64(B)))
    out
end

"""
    cmux_tree(gck, data::Array{Int32,4}, sel::AbstractMatrix, table_index=nothing; out_form=2)

CMUX-tree lookup (tfhe_cmux_tree_batch): `data` holds `T` tables of `2^depth` TLWE samples (Int32 `N x (k+1) x 2^depth x T`), `sel` is
`depth x B` (1-based indices into the loaded selectors, row 1 = the lowest address bit), `table_index` 1-based or `nothing` (first
table).  Every level replaces the pairs `(d0, d1)` by `d0 + C ⊡ (d1 - d0)` (bootstrap.jl:19-23 with tgsw.jl:125-129).  `out_form` 2
returns `Vector{LweSample}` under the gate key (tlwe.jl:55-59, keyswitch.jl:45-80), 1 the extracted samples of size `k N`, 0 the TLWE
samples as Int32 `N x (k+1) x B`.
"""
function cmux_tree(gck::GpuCloudKey, data::Array{Int32,4}, sel::AbstractMatrix, table_index=nothing; out_form::Integer=2)
    p = gck.params
    N, k = p.tlwe_polynomial_degree, p.tlwe_mask_size
    depth, B = size(sel)
    1 <= depth <= 12 || error("tfhe_mi355x: depth = ", depth, " (1 ... 12)")
    size(data)[1:3] == (N, k + 1, 1 << depth) || error("tfhe_mi355x: tables must be N x (k+1) x 2^depth x T")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    s = Matrix{Int32}(sel .- 1)
    idx = table_index === nothing ? nothing : Int32.(collect(table_index) .- 1)
    width = out_form == 2 ? p.lwe_size : k * N
    out = out_form == 0 ? Array{Int32}(undef, N, k + 1, B) : Array{Int32}(undef, width + 1, B)
    B == 0 && return out_form == 0 ? out : LweSample[]
    GC.@preserve data s idx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_cmux_tree_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int64, Int32),
        gck.ctx, data, Int64(size(data, 4)), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), Int32(depth), s, out, Int64(B), Int32(out_form)))
    out_form == 0 ? out : unflatten(out, LweParams(width))
end

"""
    cmux_net(gck, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form=2)

CMUX network (tfhe_cmux_net_batch): the CMUX of `cmux_tree` wired by a public netlist, the backward evaluation of an automaton or a
decision diagram.  `data` holds `T` tables of `E` TLWE samples (Int32 `N x (k+1) x E x T`); `widths[v]` is the node count of level `v`;
`nodes` is `3 x sum(widths)`, column `(src0, src1, var)` in level order, all 1-based: the node is `in[src0] + C_var ⊡ (in[src1] - in[src0])`
with `in` the table (first level) or the outputs of the level below, and `src0 == src1` a copy.  `sel` is `V x B` (1-based indices into
the loaded selectors), `table_index` 1-based or `nothing` (first table).  With `F = widths[end]` outputs per row, `out_form` 2 returns
the `F * B` `LweSample`s under the gate key (output `i` of row `g` at `(g - 1) F + i`), 1 the extracted samples of size `k N`, 0 the TLWE
samples as Int32 `N x (k+1) x F x B`.
"""
function cmux_net(gck::GpuCloudKey, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form::Integer=2)
    p = gck.params
    N, k = p.tlwe_polynomial_degree, p.tlwe_mask_size
    w = Int32.(collect(widths))
    levels = length(w)
    1 <= levels <= 1024 || error("tfhe_mi355x: levels = ", levels, " (1 ... 1024)")
    all(x -> 1 <= x <= 4096, w) || error("tfhe_mi355x: every width must be 1 ... 4096")
    size(nodes) == (3, sum(w)) || error("tfhe_mi355x: nodes must be 3 x sum(widths)")
    E = size(data, 3)
    size(data)[1:2] == (N, k + 1) && E >= 1 && size(data, 4) >= 1 || error("tfhe_mi355x: tables must be N x (k+1) x E x T")
    V, B = size(sel)
    V >= 1 || error("tfhe_mi355x: sel must be V x B with V >= 1")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    nd = Matrix{Int32}(nodes .- 1)
    s = Matrix{Int32}(sel .- 1)
    idx = table_index === nothing ? nothing : Int32.(collect(table_index) .- 1)
    F = Int(w[end])
    width = out_form == 2 ? p.lwe_size : k * N
    out = out_form == 0 ? Array{Int32}(undef, N, k + 1, F, B) : Array{Int32}(undef, width + 1, F * B)
    B == 0 && return out_form == 0 ? out : LweSample[]
    GC.@preserve data w nd s idx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_cmux_net_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Int64, Int32),
        gck.ctx, data, Int64(size(data, 4)), Int32(E), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), w, Int32(levels), nd, s, Int32(V), out,
        Int64(B), Int32(out_form)))
    out_form == 0 ? out : unflatten(out, LweParams(width))
end

"""
    rot_net(gck, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form=2)

CMUX network with a public monomial on every edge (tfhe_rot_net_batch): `cmux_net` with `nodes` `5 x sum(widths)`, column
`(src0, src1, var, rot0, rot1)`; the node is `X^rot0 in[src0] + C_var ⊡ (X^rot1 in[src1] - X^rot0 in[src0])` with `X^r p` the reference's
`mul_by_monomial(p, r)`.  Sources and `var` are 1-based as in `cmux_net`; the rotations are exponents in `0:2N-1` and pass unchanged.
`src0 == src1` with `rot0 == rot1` is a rotated copy, `src0 == src1` with `rot0 != rot1` a true product: the nodes
`(1, 1, b + 1, 0, 2N - 2^b)` for `b = 0 ... log2(N) - 1` bring entry `address` of a table packed `N` entries to a sample to coefficient 0,
where `out_form` 1 and 2 extract.  `data`, `sel`, `table_index` and the results are `cmux_net`'s.
"""
function rot_net(gck::GpuCloudKey, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form::Integer=2)
    p = gck.params
    N, k = p.tlwe_polynomial_degree, p.tlwe_mask_size
    w = Int32.(collect(widths))
    levels = length(w)
    1 <= levels <= 1024 || error("tfhe_mi355x: levels = ", levels, " (1 ... 1024)")
    all(x -> 1 <= x <= 4096, w) || error("tfhe_mi355x: every width must be 1 ... 4096")
    size(nodes) == (5, sum(w)) || error("tfhe_mi355x: nodes must be 5 x sum(widths)")
    all(r -> 0 <= r < 2N, view(nodes, 4:5, :)) || error("tfhe_mi355x: every rotation must be 0 ... 2N - 1")
    E = size(data, 3)
    size(data)[1:2] == (N, k + 1) && E >= 1 && size(data, 4) >= 1 || error("tfhe_mi355x: tables must be N x (k+1) x E x T")
    V, B = size(sel)
    V >= 1 || error("tfhe_mi355x: sel must be V x B with V >= 1")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    nd = Matrix{Int32}(vcat(nodes[1:3, :] .- 1, nodes[4:5, :]))
    s = Matrix{Int32}(sel .- 1)
    idx = table_index === nothing ? nothing : Int32.(collect(table_index) .- 1)
    F = Int(w[end])
    width = out_form == 2 ? p.lwe_size : k * N
    out = out_form == 0 ? Array{Int32}(undef, N, k + 1, F, B) : Array{Int32}(undef, width + 1, F * B)
    B == 0 && return out_form == 0 ? out : LweSample[]
    GC.@preserve data w nd s idx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_rot_net_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Int64, Int32),
        gck.ctx, data, Int64(size(data, 4)), Int32(E), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), w, Int32(levels), nd, s, Int32(V), out,
        Int64(B), Int32(out_form)))
    out_form == 0 ? out : unflatten(out, LweParams(width))
end

"""
    blind_rotate(gck, acc::Array{Int32,3}, rows::AbstractMatrix, sel=nothing, acc_index=nothing; in_form=0, n_out=1, out_form=2)

Blind rotation of the caller's TLWE accumulators (tfhe_blind_rotate_batch).  `acc` is `N x (k+1) x T`, TLWE samples, trivial or encrypted;
`rows` is `(steps+1) x B`, column `g` the mask words then the body of row `g`: an LWE sample (`in_form` 0) or exponents in `0:2N-1`
(`in_form` 1), which pass unchanged.  Row `g` is `A = X^(-barb) acc[acc_index[g]]` on all `k + 1` polynomials, then
`A += C_sel[i] ⊡ (X^e_i A - A)` for every step, with the selectors of `tgsw_load!` (the bootstrapping key's entries are such selectors).
`sel` (`steps` entries) and `acc_index` (`B` entries) are 1-based; `nothing` means selector `i` for step `i` and accumulator 1 for every
row.  `out_form` 0: the accumulators `N x (k+1) x B`; 1: for `j < n_out` the extraction at coefficient `j N / n_out`; 2 (default):
those keyswitched under the gate key — `n_out * B` samples, row `g`'s output `j` at `g n_out + j`.
"""
function blind_rotate(gck::GpuCloudKey, acc::Array{Int32,3}, rows::AbstractMatrix, sel=nothing, acc_index=nothing; in_form::Integer=0, n_out::Integer=1,
                      out_form::Integer=2)
    p = gck.params
    N, k = p.tlwe_polynomial_degree, p.tlwe_mask_size
    T = size(acc, 3)
    size(acc)[1:2] == (N, k + 1) && T >= 1 || error("tfhe_mi355x: accumulators must be N x (k+1) x T")
    words, B = size(rows)
    steps = words - 1
    1 <= steps <= 65536 || error("tfhe_mi355x: steps = ", steps, " (1 ... 65536)")
    0 <= in_form <= 1 || error("tfhe_mi355x: in_form = ", in_form, " (0 LWE samples, 1 exponents)")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    in_form == 0 || all(e -> 0 <= e < 2N, rows) || error("tfhe_mi355x: every exponent must be 0 ... 2N - 1")
    r = Matrix{Int32}(rows)
    s = sel === nothing ? nothing : Int32.(collect(sel) .- 1)
    s === nothing || length(s) == steps || error("tfhe_mi355x: sel must have one entry per step")
    idx = acc_index === nothing ? nothing : Int32.(collect(acc_index) .- 1)
    idx === nothing || length(idx) == B || error("tfhe_mi355x: acc_index must have one entry per row")
    width = out_form == 2 ? p.lwe_size : k * N
    out = out_form == 0 ? Array{Int32}(undef, N, k + 1, B) : Array{Int32}(undef, width + 1, n_out * B)
    B == 0 && return out_form == 0 ? out : LweSample[]
    GC.@preserve acc r s idx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_blind_rotate_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Int64, Int32),
        gck.ctx, acc, Int64(T), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), r, Int32(steps), Int32(in_form),
        s === nothing ? Ptr{Int32}(C_NULL) : pointer(s), Int32(n_out), out, Int64(B), Int32(out_form)))
    out_form == 0 ? out : unflatten(out, LweParams(width))
end

"""
    bootstrap_acc(gck, acc::Array{Int32,3}, rows::AbstractMatrix, acc_index=nothing; n_out=1, out_form=2)

`blind_rotate` on the gates' own kernel and key (tfhe_bootstrap_acc_batch): `rows` is `(n+1) x B`, LWE samples, which pass unchanged;
the steps are the context's `n` under the loaded bootstrapping key and no selector set is read.  `acc`, the 1-based `acc_index`,
`n_out`, `out_form` and the result are `blind_rotate`'s, and so are the words where the selector set holds the key's `n` entries in
order.  Served at `N = 1024`, `k = 1` (option "bootstrap_acc").  With the context's option "acc_dispatch" set to 1 (tfhe_set_option;
default 0: one wave per row at every `B`) the kernel is chosen by `B` as a gate batch's is — the multi-wave kernels for small batches,
a second launch for the last round of a large one; the words are the same.
"""
function bootstrap_acc(gck::GpuCloudKey, acc::Array{Int32,3}, rows::AbstractMatrix, acc_index=nothing; n_out::Integer=1, out_form::Integer=2)
    p = gck.params
    N, k = p.tlwe_polynomial_degree, p.tlwe_mask_size
    T = size(acc, 3)
    size(acc)[1:2] == (N, k + 1) && T >= 1 || error("tfhe_mi355x: accumulators must be N x (k+1) x T")
    words, B = size(rows)
    words == p.lwe_size + 1 || error("tfhe_mi355x: rows must be LWE samples, (n+1) x B")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    r = Matrix{Int32}(rows)
    idx = acc_index === nothing ? nothing : Int32.(collect(acc_index) .- 1)
    idx === nothing || length(idx) == B || error("tfhe_mi355x: acc_index must have one entry per row")
    width = out_form == 2 ? p.lwe_size : k * N
    out = out_form == 0 ? Array{Int32}(undef, N, k + 1, B) : Array{Int32}(undef, width + 1, n_out * B)
    B == 0 && return out_form == 0 ? out : LweSample[]
    GC.@preserve acc r idx out @locked gck.ctx check(gck.ctx, ccall((:tfhe_bootstrap_acc_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Int64),
        gck.ctx, acc, Int64(T), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), r, Int32(n_out), Int32(out_form), out, Int64(B)))
    out_form == 0 ? out : unflatten(out, LweParams(width))
end

"""
    tlwe_alloc!(gck, slots)

The device-resident TLWE table of the leveled half (tfhe_tlwe_alloc): `slots` samples of `N x (k+1)` words beside the wire table; 0 frees
it, reallocating discards the contents.  `rot_net_level!` and `blind_rotate_level!` read and write it; slots are 1-based here.
"""
function tlwe_alloc!(gck::GpuCloudKey, slots::Integer)
    slots >= 0 || error("tfhe_mi355x: slots = ", slots, " (at least 0)")
    @locked gck.ctx check(gck.ctx, ccall((:tfhe_tlwe_alloc, LIB), Int32, (Ptr{Cvoid}, Int64), gck.ctx, Int64(slots)))
    gck
end

"""
    tlwe_upload!(gck, first, samples::Array{Int32,3})

`samples`, `N x (k+1) x count`, into slots `first : first + count - 1` (1-based) of the TLWE table (tfhe_tlwe_upload), behind the levels
queued on the context.
"""
function tlwe_upload!(gck::GpuCloudKey, first::Integer, samples::Array{Int32,3})
    p = gck.params
    N, k = p.tlwe_polynomial_degree, p.tlwe_mask_size
    size(samples)[1:2] == (N, k + 1) || error("tfhe_mi355x: TLWE samples must be N x (k+1) x count")
    first >= 1 || error("tfhe_mi355x: slots are 1-based, first = ", first)
    GC.@preserve samples @locked gck.ctx check(gck.ctx, ccall((:tfhe_tlwe_upload, LIB), Int32,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}), gck.ctx, Int64(first - 1), Int64(size(samples, 3)), samples))
    gck
end

"""
    tlwe_download(gck, first, count)  ->  Array{Int32,3}

Slots `first : first + count - 1` (1-based) of the TLWE table as `N x (k+1) x count` (tfhe_tlwe_download), behind the levels queued on
the context.
"""
function tlwe_download(gck::GpuCloudKey, first::Integer, count::Integer)
    p = gck.params
    N, k = p.tlwe_polynomial_degree, p.tlwe_mask_size
    first >= 1 && count >= 0 || error("tfhe_mi355x: slots are 1-based and count >= 0, got first = ", first, ", count = ", count)
    out = Array{Int32}(undef, N, k + 1, count)
    GC.@preserve out @locked gck.ctx check(gck.ctx, ccall((:tfhe_tlwe_download, LIB), Int32,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}), gck.ctx, Int64(first - 1), Int64(count), out))
    out
end

"""
    tgsw_update!(gck, first, tgsw::Array{Int32})

Replaces selectors `first : first + count - 1` (1-based) of the set `tgsw_load!` loaded, in place (tfhe_tgsw_update); `tgsw` as in
`tgsw_load!`.  Every other selector keeps its words: the key's `n` selectors are loaded once, a request's address bits swapped behind them.
"""
function tgsw_update!(gck::GpuCloudKey, first::Integer, tgsw::Array{Int32})
    p = gck.params
    per = p.tlwe_polynomial_degree * (p.tlwe_mask_size + 1)^2 * p.bs_decomp_length
    (length(tgsw) > 0 && length(tgsw) % per == 0) || error("tfhe_mi355x: TGSW samples must hold a positive multiple of ", per, " words")
    first >= 1 || error("tfhe_mi355x: selectors are 1-based, first = ", first)
    GC.@preserve tgsw @locked gck.ctx check(gck.ctx, ccall((:tfhe_tgsw_update, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Int64), gck.ctx, tgsw, Int64(first - 1), Int64(length(tgsw) ÷ per)))
    gck
end

"""
    rot_net_level!(gck, E, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_first=nothing; out_form=2, out_first=1, out_wires=nothing)

`rot_net` between the device-resident tables (tfhe_rot_net_level).  Level 0 of row `g` reads source `src` at TLWE slot
`table_first[g] + src - 1` (`table_first` 1-based, `B` entries; `nothing`: `src` is an absolute slot); `E`, `widths`, `nodes`, `sel` as in
`rot_net`.  `out_form` 0: output node `i` of row `g` goes to slot `out_first + (g - 1) F + i - 1`; `out_form` 2: keyswitched, to wire
`out_wires[(g - 1) F + i]` (1-based wires of the wire table).  The words are `rot_net`'s on the same samples.  Synchronous.
"""
function rot_net_level!(gck::GpuCloudKey, E::Integer, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_first=nothing; out_form::Integer=2,
                        out_first::Integer=1, out_wires=nothing)
    N = gck.params.tlwe_polynomial_degree
    w = Int32.(collect(widths))
    levels = length(w)
    1 <= levels <= 1024 || error("tfhe_mi355x: levels = ", levels, " (1 ... 1024)")
    all(x -> 1 <= x <= 4096, w) || error("tfhe_mi355x: every width must be 1 ... 4096")
    size(nodes) == (5, sum(w)) || error("tfhe_mi355x: nodes must be 5 x sum(widths)")
    all(r -> 0 <= r < 2N, view(nodes, 4:5, :)) || error("tfhe_mi355x: every rotation must be 0 ... 2N - 1")
    E >= 1 || error("tfhe_mi355x: E = ", E, " (at least one entry)")
    V, B = size(sel)
    V >= 1 || error("tfhe_mi355x: sel must be V x B with V >= 1")
    out_form == 0 || out_form == 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 into TLWE slots, 2 key-switched into wires)")
    nd = Matrix{Int32}(vcat(nodes[1:3, :] .- 1, nodes[4:5, :]))
    s = Matrix{Int32}(sel .- 1)
    tf = table_first === nothing ? nothing : Int32.(collect(table_first) .- 1)
    tf === nothing || length(tf) == B || error("tfhe_mi355x: table_first must have one entry per row")
    F = Int(w[end])
    ow = out_wires === nothing ? nothing : Int32.(collect(out_wires) .- 1)
    out_form != 2 || (ow !== nothing && length(ow) == F * B) || error("tfhe_mi355x: out_wires must have F * B entries with out_form 2")
    out_form != 0 || out_first >= 1 || error("tfhe_mi355x: slots are 1-based, out_first = ", out_first)
    GC.@preserve w nd s tf ow @locked gck.ctx check(gck.ctx, ccall((:tfhe_rot_net_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Int64, Ptr{Int32}, Int64),
        gck.ctx, tf === nothing ? Ptr{Int32}(C_NULL) : pointer(tf), Int32(E), w, Int32(levels), nd, s, Int32(V), Int32(out_form), Int64(out_first - 1),
        ow === nothing ? Ptr{Int32}(C_NULL) : pointer(ow), Int64(B)))
    gck
end

"""
    blind_rotate_level!(gck, acc_slot, term_start, term_wire, term_coef; cst=nothing, sel=nothing, n_out=1, out_form=2, out_slot=nothing, out_wires=nothing)

`blind_rotate` between the device-resident tables (tfhe_blind_rotate_level).  Row `g` rotates the sample in TLWE slot `acc_slot[g]` by the
LWE sample `sum_t term_coef[t] * wire[term_wire[t]] + cst[g]` over the terms `term_start[g] + 1 : term_start[g + 1]` (`term_start` is the
0-based prefix sum of the rows' term counts, `B + 1` entries from 0, as tfhe_lut_level takes it; it and the coefficients pass unchanged;
slots, wires and selectors are 1-based), over the context's `n` steps on the selectors `sel` (`nothing`: selector `i` for step `i`).
`out_form` 0 (`n_out` 1): the final accumulator goes to slot `out_slot[g]`; `out_form` 2: the `n_out` extractions, keyswitched, go to
wires `out_wires[(g - 1) n_out + j]`.  The words are `blind_rotate`'s on the same samples.  Synchronous.
"""
function blind_rotate_level!(gck::GpuCloudKey, acc_slot, term_start, term_wire, term_coef; cst=nothing, sel=nothing, n_out::Integer=1,
                             out_form::Integer=2, out_slot=nothing, out_wires=nothing)
    p = gck.params
    N = p.tlwe_polynomial_degree
    acc = Int32.(collect(acc_slot) .- 1)
    B = length(acc)
    start = Int32.(collect(term_start))
    length(start) == B + 1 && start[1] == 0 && issorted(start) || error("tfhe_mi355x: term_start must be B + 1 non-decreasing entries from 0")
    T = Int(start[end])
    tw = Int32.(collect(term_wire) .- 1)
    tc = Int32.(collect(term_coef))
    length(tw) >= T && length(tc) >= T || error("tfhe_mi355x: term_wire and term_coef must have term_start[end] entries")
    c = cst === nothing ? nothing : Int32.(collect(cst))
    c === nothing || length(c) == B || error("tfhe_mi355x: cst must have one entry per row")
    s = sel === nothing ? nothing : Int32.(collect(sel) .- 1)
    s === nothing || length(s) == p.lwe_size || error("tfhe_mi355x: sel must have one entry per step (n)")
    out_form == 0 || out_form == 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 into TLWE slots, 2 key-switched into wires)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    os = out_slot === nothing ? nothing : Int32.(collect(out_slot) .- 1)
    ow = out_wires === nothing ? nothing : Int32.(collect(out_wires) .- 1)
    out_form != 0 || (os !== nothing && length(os) == B) || error("tfhe_mi355x: out_slot must have one entry per row with out_form 0")
    out_form != 2 || (ow !== nothing && length(ow) == n_out * B) || error("tfhe_mi355x: out_wires must have n_out * B entries with out_form 2")
    GC.@preserve acc start tw tc c s os ow @locked gck.ctx check(gck.ctx, ccall((:tfhe_blind_rotate_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Int64),
        gck.ctx, acc, start, tw, tc, c === nothing ? Ptr{Int32}(C_NULL) : pointer(c), s === nothing ? Ptr{Int32}(C_NULL) : pointer(s), Int32(n_out),
        Int32(out_form), os === nothing ? Ptr{Int32}(C_NULL) : pointer(os), ow === nothing ? Ptr{Int32}(C_NULL) : pointer(ow), Int64(B)))
    gck
end

"""
    bootstrap_acc_level!(gck, acc_slot, term_start, term_wire, term_coef; cst=nothing, n_out=1, out_form=2, out_slot=nothing, out_wires=nothing)

`bootstrap_acc` between the device-resident tables (tfhe_bootstrap_acc_level): `blind_rotate_level!` on the gates' own kernel and key,
without a selector set.  Every argument, the 1-based slots and wires and the words are `blind_rotate_level!`'s with `sel = nothing`.
Synchronous.  The context's option "acc_dispatch" (see `bootstrap_acc`) chooses the kernel by the number of rows; the words are the same.
"""
function bootstrap_acc_level!(gck::GpuCloudKey, acc_slot, term_start, term_wire, term_coef; cst=nothing, n_out::Integer=1, out_form::Integer=2,
                              out_slot=nothing, out_wires=nothing)
    p = gck.params
    N = p.tlwe_polynomial_degree
    acc = Int32.(collect(acc_slot) .- 1)
    B = length(acc)
    start = Int32.(collect(term_start))
    length(start) == B + 1 && start[1] == 0 && issorted(start) || error("tfhe_mi355x: term_start must be B + 1 non-decreasing entries from 0")
    T = Int(start[end])
    tw = Int32.(collect(term_wire) .- 1)
    tc = Int32.(collect(term_coef))
    length(tw) >= T && length(tc) >= T || error("tfhe_mi355x: term_wire and term_coef must have term_start[end] entries")
    c = cst === nothing ? nothing : Int32.(collect(cst))
    c === nothing || length(c) == B || error("tfhe_mi355x: cst must have one entry per row")
    out_form == 0 || out_form == 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 into TLWE slots, 2 key-switched into wires)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    os = out_slot === nothing ? nothing : Int32.(collect(out_slot) .- 1)
    ow = out_wires === nothing ? nothing : Int32.(collect(out_wires) .- 1)
    out_form != 0 || (os !== nothing && length(os) == B) || error("tfhe_mi355x: out_slot must have one entry per row with out_form 0")
    out_form != 2 || (ow !== nothing && length(ow) == n_out * B) || error("tfhe_mi355x: out_wires must have n_out * B entries with out_form 2")
    GC.@preserve acc start tw tc c os ow @locked gck.ctx check(gck.ctx, ccall((:tfhe_bootstrap_acc_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Int64),
        gck.ctx, acc, start, tw, tc, c === nothing ? Ptr{Int32}(C_NULL) : pointer(c), Int32(n_out),
        Int32(out_form), os === nothing ? Ptr{Int32}(C_NULL) : pointer(os), ow === nothing ? Ptr{Int32}(C_NULL) : pointer(ow), Int64(B)))
    gck
end

# page-locked Int32 matrix (tfhe_host_alloc): the copies of a streamed batch are then single DMA transfers that overlap kernels
function pinned_matrix(rows::Int, cols::Int)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:tfhe_host_alloc, LIB), Int32, (Csize_t, Ptr{Ptr{Cvoid}}), Csize_t(4 * rows * cols), p)
    rc == 0 || error("tfhe_mi355x: tfhe_host_alloc failed (", rc, ")")
    unsafe_wrap(Array, Ptr{Int32}(p[]), (rows, cols); own=false)
end
release_pinned(a::Array{Int32}) = ccall((:tfhe_host_free, LIB), Cvoid, (Ptr{Cvoid},), pointer(a))

"""
    t = gates_batch_async(gck, opcodes, xs, ys=nothing, zs=nothing)  ->  PendingGates
    fetch(t)                                                         ->  Vector{LweSample}

Streaming form of `gates_batch` (tfhe_gates_batch_submit / tfhe_gates_batch_wait): the call returns once the batch is
enqueued; up to two batches run at a time, the upload of one under the kernels of the other, so a caller that feeds
batch after batch pays no PCIe time in the steady state.  Operands are staged in page-locked buffers that `fetch` frees.
"""
mutable struct PendingGates
    key::GpuCloudKey
    ticket::Int32
    buffers::Vector{Array{Int32}}     # page-locked operand copies + the result, alive until fetch
    out::Array{Int32}
    done::Bool
end

function gates_batch_async(gck::GpuCloudKey, opcodes::Vector{UInt8}, xs, ys=nothing, zs=nothing)
    B = length(opcodes)
    B > 0 || error("gates_batch_async: empty batch")
    n1 = gck.params.lwe_size + 1
    stage(v) = v === nothing ? nothing : copyto!(pinned_matrix(n1, B), flatten(v))
    fx, fy, fz = stage(xs), stage(ys), stage(zs)
    out = pinned_matrix(n1, B)
    ptr(a) = a === nothing ? Ptr{Int32}(C_NULL) : pointer(a)
    ticket = Ref{Int32}(-1)
    bufs = Array{Int32}[b for b in (fx, fy, fz, out) if b !== nothing]
    rc = @locked gck.ctx ccall((:tfhe_gates_batch_submit, LIB), Int32,
        (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Int32}),
        gck.ctx, opcodes, ptr(fx), ptr(fy), ptr(fz), out, B, ticket)
    if rc != 0
        foreach(release_pinned, bufs)
        @locked gck.ctx check(gck.ctx, rc)
    end
    t = PendingGates(gck, ticket[], bufs, out, false)
    # a PendingGates that is dropped (or whose fetch is never reached) must not leak its page-locked buffers: wait for the
    # batch, then free them (a finalizer may call into C; it must not allocate Julia objects, and this one does not)
    finalizer(abandon!, t)
    t
end

# Runs as a finalizer: it cannot take the context's lock, and another task may be inside a gate call on the same context at
# this very moment.  tfhe_ctx_synchronize (ABI v7) is the one entry point made for that: it takes no ownership of the context,
# touches none of its state and returns once everything queued so far — this batch's copies included — has completed.  The
# page-locked buffers go back ONLY after it returned TFHE_OK: on any other answer they are leaked rather than freed under a DMA
# that may still be running.  (Until ABI v6 this called tfhe_gates_batch_wait, which the library's one-caller-at-a-time guard
# answered with TFHE_ERR_STATE at once while another task was inside a call — and the buffers were freed regardless.)
function abandon!(t::PendingGates)
    t.done && return nothing
    drained = t.key.ctx == C_NULL ||      # (the context is gone: tfhe_ctx_destroy synchronised its streams)
              ccall((:tfhe_ctx_synchronize, LIB), Int32, (Ptr{Cvoid},), t.key.ctx) == 0
    drained && foreach(release_pinned, t.buffers)
    empty!(t.buffers)
    t.done = true
    nothing
end

function Base.fetch(t::PendingGates)
    t.done && error("PendingGates: already fetched")
    rc = @locked t.key.ctx ccall((:tfhe_gates_batch_wait, LIB), Int32, (Ptr{Cvoid}, Int32), t.key.ctx, t.ticket)
    # a failed wait says nothing about the copies still in flight: drain the context (tfhe_ctx_synchronize needs no lock and
    # cannot be refused) before the buffers go back; if even that fails they are leaked, not freed under a live DMA
    drained = rc == 0 || ccall((:tfhe_ctx_synchronize, LIB), Int32, (Ptr{Cvoid},), t.key.ctx) == 0
    res = rc == 0 ? unflatten(copy(t.out), LweParams(t.key.params.lwe_size)) : nothing
    drained && foreach(release_pinned, t.buffers)
    empty!(t.buffers)
    t.done = true
    check(t.key.ctx, rc)
    res
end

# one level of B gates on device-resident operands (tfhe_gates_level); host samples among them are uploaded first
function gates_on_device(g::GpuCloudKey, op::UInt8, operands)
    B = batch_length(operands)
    devs = map(operands) do x
        d = x isa GpuLweArray ? x : upload(g, x isa LweSample ? [x] : x)
        d.key === g || error("GpuLweArray belongs to another GpuCloudKey")
        d
    end
    index(d) = length(d) == B ? d.rows : fill(d.rows[1], B)
    ia = index(devs[1])
    ib = length(devs) >= 2 ? index(devs[2]) : Int32[]
    ic = length(devs) >= 3 ? index(devs[3]) : Int32[]
    out = alloc_rows!(g, B)
    opcodes = fill(op, B)
    ptr(a) = isempty(a) ? Ptr{Int32}(C_NULL) : pointer(a)
    GC.@preserve opcodes ia ib ic out devs @locked g.ctx check(g.ctx, ccall((:tfhe_gates_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64),
        g.ctx, opcodes, ptr(ia), ptr(ib), ptr(ic), out, B))
    GpuLweArray(g, out)
end

# One gate kind over scalar / vector / device operands: all LweSample -> a LweSample (batch of one); any vector ->
# Vector{LweSample} from ONE tfhe_gates_batch; any GpuLweArray -> a GpuLweArray (nothing leaves the device).
function run_gate(g::GpuCloudKey, op::UInt8, operands...)
    any(x -> x isa GpuLweArray, operands) && return gates_on_device(g, op, operands)
    B = batch_length(operands)
    vecs = map(x -> expand(x, B), operands)
    res = gates_batch(g, fill(op, B), vecs...)
    all(x -> x isa LweSample, operands) ? res[1] : res
end

# Methods ON TFHE's functions (src/gates.jl:15-153), and the batched forms of their broadcast: gate_xor.(gck, c1, c2)
# (docs/src/manual.md:35) lowers to broadcasted(gate_xor, gck, c1, c2), which these methods answer with one GPU call
# instead of length(c1) single-gate launches.
for (fn, op) in ((:gate_nand, NAND), (:gate_or, OR), (:gate_and, AND), (:gate_xor, XOR),
                 (:gate_xnor, XNOR), (:gate_nor, NOR), (:gate_andny, ANDNY), (:gate_andyn, ANDYN),
                 (:gate_orny, ORNY), (:gate_oryn, ORYN))
    @eval begin
        $fn(g::GpuCloudKey, x::LweOperand, y::LweOperand) = run_gate(g, $op, x, y)
        broadcasted(::typeof($fn), g::GpuCloudKey, x::LweOperand, y::LweOperand) = run_gate(g, $op, x, y)
        broadcasted(::typeof($fn), g::Base.RefValue{GpuCloudKey}, x::LweOperand, y::LweOperand) = run_gate(g[], $op, x, y)
    end
end

# src/gates.jl:163-177
gate_mux(g::GpuCloudKey, x::LweOperand, y::LweOperand, z::LweOperand) = run_gate(g, MUX, x, y, z)
broadcasted(::typeof(gate_mux), g::GpuCloudKey, x::LweOperand, y::LweOperand, z::LweOperand) = run_gate(g, MUX, x, y, z)
broadcasted(::typeof(gate_mux), g::Base.RefValue{GpuCloudKey}, x::LweOperand, y::LweOperand, z::LweOperand) =
    run_gate(g[], MUX, x, y, z)

# not bootstrapped (src/gates.jl:76-93): on host samples no device round trip is needed
gate_not(g::GpuCloudKey, x::LweSample) = -x
gate_not(g::GpuCloudKey, xs::LweVec) = [-x for x in xs]
gate_not(g::GpuCloudKey, d::GpuLweArray) = gates_on_device(g, NOT, (d,))
broadcasted(::typeof(gate_not), g::GpuCloudKey, x::LweOperand) = gate_not(g, x)
broadcasted(::typeof(gate_not), g::Base.RefValue{GpuCloudKey}, x::LweOperand) = gate_not(g[], x)

gate_constant(g::GpuCloudKey, value::Bool) =
    TFHE.lwe_noiseless_trivial(TFHE.encode_message(value ? 1 : -1, 8), LweParams(g.params.lwe_size))
broadcasted(::typeof(gate_constant), g::GpuCloudKey, values::AbstractVector{Bool}) = [gate_constant(g, v) for v in values]
broadcasted(::typeof(gate_constant), g::Base.RefValue{GpuCloudKey}, values::AbstractVector{Bool}) =
    [gate_constant(g[], v) for v in values]

# ---- multi-key (src/mk_api.jl:83-101, src/mk_gates.jl:7-12) ---------------------------------------------------
# MKBootstrapKey.key[j, i] (bit j of party i) :: MKTransformedTGswExpSample with spectra x[l, P], y[l, P], c0[l],
# c1[l] (src/mk_internals.jl:274-288, 442-461) -> complex128, C order [P][n][2lP + 2l][N/2], per (i, j) the polys
# x[p, q] at (p-1)*P + q, then y, then c0, then c1 (include/tfhe_mi355x.h).
function flatten_mk_spectra(bk, p::SchemeParameters, parties::Int)
    n, l, M = p.lwe_size, p.bs_decomp_length, p.tlwe_polynomial_degree ÷ 2
    per = 2 * l * parties + 2 * l
    spectra = Array{Complex{Float64}}(undef, M, per, n, parties)      # column-major: M fastest
    for i in 1:parties, j in 1:n
        s = bk.key[j, i]
        for pp in 1:l, q in 1:parties
            spectra[:, (pp - 1) * parties + q, j, i] .= s.x[pp, q].coeffs
            spectra[:, l * parties + (pp - 1) * parties + q, j, i] .= s.y[pp, q].coeffs
        end
        for pp in 1:l
            spectra[:, 2 * l * parties + pp, j, i] .= s.c0[pp].coeffs
            spectra[:, 2 * l * parties + l + pp, j, i] .= s.c1[pp].coeffs
        end
    end
    spectra
end

"""
    GpuMKCloudKey(ck::MKCloudKey; device=0, devices=nothing)

An `MKCloudKey` resident on the GPU(s); pass it to TFHE's own `mk_gate_nand` in place of the `MKCloudKey`.
"""
mutable struct GpuMKCloudKey
    params::SchemeParameters
    parties::Int
    ctx::Ptr{Cvoid}

    function GpuMKCloudKey(ck::MKCloudKey; device::Integer=0, devices=nothing)
        p, P = ck.params, ck.parties
        ctx = create_context(p, devices === nothing ? [device] : devices)
        mck = new(p, P, ctx)
        finalizer(destroy!, mck)
        try
            spectra = flatten_mk_spectra(ck.bootstrap_key, p, P)
            GC.@preserve spectra @locked ctx check(ctx, ccall((:tfhe_mk_load_bootstrap_key_c128, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Complex{Float64}}, Int32), ctx, spectra, Int32(P)))
            # P single-key keyswitch keys back to back (src/mk_api.jl:97-98)
            flat = cat([flatten_keyswitch_key(ks, p.lwe_size) for ks in ck.keyswitch_key]...; dims=5)
            GC.@preserve flat @locked ctx check(ctx, ccall((:tfhe_mk_load_keyswitch_key, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Int32}, Int32), ctx, flat, Int32(P)))
        catch
            destroy!(mck)
            rethrow()
        end
        mck
    end
end

broadcastable(m::GpuMKCloudKey) = Ref(m)

# MKLweSample (src/mk_internals.jl:6-18: a is n x P, one column per party) <-> flat Int32[P*n+1] = a[:,1]; a[:,2]; ...; b
function flatten(xs::AbstractVector{MKLweSample})
    n, P = size(xs[1].a)
    m = Array{Int32}(undef, n * P + 1, length(xs))
    for (g, x) in enumerate(xs)
        m[1:n*P, g] .= vec(x.a)                                        # column-major vec = party columns in order
        m[n * P + 1, g] = x.b
    end
    m
end

const MKVec = AbstractVector{MKLweSample}

function mk_nand_batch(mck::GpuMKCloudKey, xs::MKVec, ys::MKVec)
    length(xs) == length(ys) || throw(DimensionMismatch("mk_gate_nand operands of lengths $(length(xs)) and $(length(ys))"))
    n, P, B = mck.params.lwe_size, mck.parties, length(xs)
    fx, fy = flatten(xs), flatten(ys)
    out = Array{Int32}(undef, n * P + 1, B)
    GC.@preserve fx fy out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_gate_nand_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64), mck.ctx, fx, fy, out, B))
    params = LweParams(n)
    # current_variance: 0.0 as the reference's own TODO leaves it (src/mk_internals.jl:94)
    [MKLweSample(params, reshape(out[1:n*P, g], n, P), out[n * P + 1, g], 0.) for g in 1:B]
end

# methods on TFHE's mk_gate_nand (src/mk_gates.jl:7-12): scalar, vectors, and the batched form of its broadcast
mk_gate_nand(mck::GpuMKCloudKey, x::MKLweSample, y::MKLweSample) = mk_nand_batch(mck, [x], [y])[1]
mk_gate_nand(mck::GpuMKCloudKey, xs::MKVec, ys::MKVec) = mk_nand_batch(mck, xs, ys)
broadcasted(::typeof(mk_gate_nand), mck::GpuMKCloudKey, xs::MKVec, ys::MKVec) = mk_nand_batch(mck, xs, ys)
broadcasted(::typeof(mk_gate_nand), mck::Base.RefValue{GpuMKCloudKey}, xs::MKVec, ys::MKVec) = mk_nand_batch(mck[], xs, ys)

"""
    mk_tgsw_load!(mck, tgsw::Array{Int32}, party_of)

The selector set of `mk_extern_mul` / `mk_cmux_tree` (tfhe_mk_tgsw_load): `S` expanded RGSW samples (`mk_tgsw_expand`,
src/mk_internals.jl:304-345) as Int32 `N x (2lP + 2l) x S` (column-major: the C layout [S][2lP + 2l][N], per sample `x[l][P]`,
`y[l][P]`, `c0[l]`, `c1[l]` as in the multi-key bootstrapping key) and `party_of[s]` (1-based), the party sample `s` was expanded
for.  Replaces any earlier set.
"""
function mk_tgsw_load!(mck::GpuMKCloudKey, tgsw::Array{Int32}, party_of)
    p, P = mck.params, mck.parties
    per = p.tlwe_polynomial_degree * (2 * p.bs_decomp_length * P + 2 * p.bs_decomp_length)
    who = Int32.(collect(party_of) .- 1)
    (length(who) > 0 && length(tgsw) == per * length(who)) || error("tfhe_mi355x: expanded samples must hold ", per, " words for each entry of party_of")
    GC.@preserve tgsw who @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_tgsw_load, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int64, Int32), mck.ctx, tgsw, who, Int64(length(who)), Int32(P)))
    mck
end

"""
    mk_extern_mul(mck, tlwe::Array{Int32,3}, sel)  ->  Array{Int32,3}

`mk_tgsw_extern_mul` (src/mk_internals.jl:348-391) for a batch (tfhe_mk_extern_mul_batch): MK TLWE sample `g` of `tlwe` (Int32
`N x (P+1) x B`: the party masks, then the body) times loaded selector `sel[g]` (1-based).
"""
function mk_extern_mul(mck::GpuMKCloudKey, tlwe::Array{Int32,3}, sel)
    p, P = mck.params, mck.parties
    size(tlwe)[1:2] == (p.tlwe_polynomial_degree, P + 1) || error("tfhe_mi355x: MK TLWE samples must be N x (P+1) x B")
    B = size(tlwe, 3)
    idx = Int32.(collect(sel) .- 1)
    length(idx) == B || error("tfhe_mi355x: one selector per sample")
    out = similar(tlwe)
    B == 0 && return out
    GC.@preserve tlwe idx out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_extern_mul_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64), mck.ctx, tlwe, idx, out, Int64(B)))
    out
end

"""
    mk_cmux_tree(mck, data::Array{Int32,4}, sel::AbstractMatrix, table_index=nothing; out_form=2)

CMUX-tree lookup on multi-key samples (tfhe_mk_cmux_tree_batch): `cmux_tree` with tables Int32 `N x (P+1) x 2^depth x T`; every level
is `d0 + C ⊡ (d1 - d0)`, the form of `mk_mux_rotate` (src/mk_internals.jl:464-471) without the monomial.  `out_form` 2 returns
`Vector{MKLweSample}` (mk_tlwe_extract_sample :88-95, mk_keyswitch :397-411) that `mk_gate_nand` accepts, 1 the extracted samples as
Int32 `(P N + 1) x B`, 0 the MK TLWE samples as Int32 `N x (P+1) x B`.
"""
function mk_cmux_tree(mck::GpuMKCloudKey, data::Array{Int32,4}, sel::AbstractMatrix, table_index=nothing; out_form::Integer=2)
    p, P = mck.params, mck.parties
    N, n = p.tlwe_polynomial_degree, p.lwe_size
    depth, B = size(sel)
    1 <= depth <= 12 || error("tfhe_mi355x: depth = ", depth, " (1 ... 12)")
    size(data)[1:3] == (N, P + 1, 1 << depth) || error("tfhe_mi355x: tables must be N x (P+1) x 2^depth x T")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    s = Matrix{Int32}(sel .- 1)
    idx = table_index === nothing ? nothing : Int32.(collect(table_index) .- 1)
    width = out_form == 2 ? P * n : P * N
    out = out_form == 0 ? Array{Int32}(undef, N, P + 1, B) : Array{Int32}(undef, width + 1, B)
    B == 0 && return out_form == 2 ? MKLweSample[] : out
    GC.@preserve data s idx out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_cmux_tree_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int64, Int32),
        mck.ctx, data, Int64(size(data, 4)), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), Int32(depth), s, out, Int64(B), Int32(out_form)))
    out_form == 2 || return out
    params = LweParams(n)
    [MKLweSample(params, reshape(out[1:n*P, g], n, P), out[n * P + 1, g], 0.) for g in 1:B]
end

"""
    mk_cmux_net(mck, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form=2)

CMUX network on multi-key samples (tfhe_mk_cmux_net_batch): `cmux_net` with tables Int32 `N x (P+1) x E x T` and `sel` (`V x B`, 1-based)
into the selectors of `mk_tgsw_load!`; every node multiplies for the party of its own selector, so the comparison of two integers that
two parties hold is the comparator network on their uni-encrypted bits.  `widths`, `nodes` (`3 x sum(widths)`, 1-based) and
`table_index` as `cmux_net`.  With `F = widths[end]` outputs per row, `out_form` 2 returns the `F * B` `MKLweSample`s that `mk_gate_nand`
accepts (output `i` of row `g` at `(g - 1) F + i`), 1 the extracted samples as Int32 `(P N + 1) x (F B)`, 0 the MK TLWE samples as Int32
`N x (P+1) x F x B`.
"""
function mk_cmux_net(mck::GpuMKCloudKey, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form::Integer=2)
    p, P = mck.params, mck.parties
    N, n = p.tlwe_polynomial_degree, p.lwe_size
    w = Int32.(collect(widths))
    levels = length(w)
    1 <= levels <= 1024 || error("tfhe_mi355x: levels = ", levels, " (1 ... 1024)")
    all(x -> 1 <= x <= 4096, w) || error("tfhe_mi355x: every width must be 1 ... 4096")
    size(nodes) == (3, sum(w)) || error("tfhe_mi355x: nodes must be 3 x sum(widths)")
    E = size(data, 3)
    size(data)[1:2] == (N, P + 1) && E >= 1 && size(data, 4) >= 1 || error("tfhe_mi355x: tables must be N x (P+1) x E x T")
    V, B = size(sel)
    V >= 1 || error("tfhe_mi355x: sel must be V x B with V >= 1")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    nd = Matrix{Int32}(nodes .- 1)
    s = Matrix{Int32}(sel .- 1)
    idx = table_index === nothing ? nothing : Int32.(collect(table_index) .- 1)
    F = Int(w[end])
    width = out_form == 2 ? P * n : P * N
    out = out_form == 0 ? Array{Int32}(undef, N, P + 1, F, B) : Array{Int32}(undef, width + 1, F * B)
    B == 0 && return out_form == 2 ? MKLweSample[] : out
    GC.@preserve data w nd s idx out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_cmux_net_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Int64, Int32),
        mck.ctx, data, Int64(size(data, 4)), Int32(E), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), w, Int32(levels), nd, s, Int32(V), out,
        Int64(B), Int32(out_form)))
    out_form == 2 || return out
    params = LweParams(n)
    [MKLweSample(params, reshape(out[1:n*P, r], n, P), out[n * P + 1, r], 0.) for r in 1:F*B]
end

"""
    mk_rot_net(mck, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form=2)

CMUX network with a public monomial on every edge, on multi-key samples (tfhe_mk_rot_net_batch): `mk_cmux_net` with `nodes`
`5 x sum(widths)`, column `(src0, src1, var, rot0, rot1)`; the node is `X^rot0 in[src0] + C_var ⊡ (X^rot1 in[src1] - X^rot0 in[src0])` with
`X^r` the reference's `mul_by_monomial` on all `P + 1` polynomials and the product for the party of selector `var`.  Sources and `var` are
1-based as in `mk_cmux_net`; the rotations are exponents in `0:2N-1` and pass unchanged.  The nodes `(1, 1, b + 1, 0, 2N - 2^b)` for
`b = 0 ... log2(N) - 1` read a table packed `N` entries to an MK TLWE sample at an address whose bits several parties own.  `data`,
`sel`, `table_index` and the results are `mk_cmux_net`'s.
"""
function mk_rot_net(mck::GpuMKCloudKey, data::Array{Int32,4}, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_index=nothing; out_form::Integer=2)
    p, P = mck.params, mck.parties
    N, n = p.tlwe_polynomial_degree, p.lwe_size
    w = Int32.(collect(widths))
    levels = length(w)
    1 <= levels <= 1024 || error("tfhe_mi355x: levels = ", levels, " (1 ... 1024)")
    all(x -> 1 <= x <= 4096, w) || error("tfhe_mi355x: every width must be 1 ... 4096")
    size(nodes) == (5, sum(w)) || error("tfhe_mi355x: nodes must be 5 x sum(widths)")
    all(r -> 0 <= r < 2N, view(nodes, 4:5, :)) || error("tfhe_mi355x: every rotation must be 0 ... 2N - 1")
    E = size(data, 3)
    size(data)[1:2] == (N, P + 1) && E >= 1 && size(data, 4) >= 1 || error("tfhe_mi355x: tables must be N x (P+1) x E x T")
    V, B = size(sel)
    V >= 1 || error("tfhe_mi355x: sel must be V x B with V >= 1")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    nd = Matrix{Int32}(vcat(nodes[1:3, :] .- 1, nodes[4:5, :]))
    s = Matrix{Int32}(sel .- 1)
    idx = table_index === nothing ? nothing : Int32.(collect(table_index) .- 1)
    F = Int(w[end])
    width = out_form == 2 ? P * n : P * N
    out = out_form == 0 ? Array{Int32}(undef, N, P + 1, F, B) : Array{Int32}(undef, width + 1, F * B)
    B == 0 && return out_form == 2 ? MKLweSample[] : out
    GC.@preserve data w nd s idx out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_rot_net_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Int64, Int32),
        mck.ctx, data, Int64(size(data, 4)), Int32(E), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), w, Int32(levels), nd, s, Int32(V), out,
        Int64(B), Int32(out_form)))
    out_form == 2 || return out
    params = LweParams(n)
    [MKLweSample(params, reshape(out[1:n*P, r], n, P), out[n * P + 1, r], 0.) for r in 1:F*B]
end

"""
    mk_blind_rotate(mck, acc::Array{Int32,3}, rows::AbstractMatrix, sel=nothing, acc_index=nothing; in_form=0, n_out=1, out_form=2)

Multi-key blind rotation of the caller's MK TLWE accumulators (tfhe_mk_blind_rotate_batch): `blind_rotate` under a multi-key cloud key.
`acc` is `N x (P+1) x T`, MK TLWE samples, trivial or encrypted; `rows` is `(steps+1) x B`, column `g` the step words then the body of row
`g`: a multi-key LWE sample as it lies in memory (`in_form` 0) or exponents in `0:2N-1` (`in_form` 1), which pass unchanged.  Row `g` is
`A = X^(-barb) acc[acc_index[g]]` on all `P + 1` polynomials, then `A += C_sel[i] ⊡ (X^e_i A - A)` for every step, with the selectors of
`mk_tgsw_load!` and the product for the party of selector `sel[i]` (the `(party, bit)` entries of the multi-key bootstrapping key are
such selectors).  `sel` (`steps` entries) and `acc_index` (`B` entries) are 1-based; `nothing` means selector `i` for step `i` and
accumulator 1 for every row.  `out_form` 0: the accumulators `N x (P+1) x B`; 1: for `j < n_out` the extraction at coefficient
`j N / n_out`, `(P N + 1) x n_out B`; 2 (default): those keyswitched — `n_out * B` `MKLweSample`s, row `g`'s output `j` at `g n_out + j`.
"""
function mk_blind_rotate(mck::GpuMKCloudKey, acc::Array{Int32,3}, rows::AbstractMatrix, sel=nothing, acc_index=nothing; in_form::Integer=0,
                         n_out::Integer=1, out_form::Integer=2)
    p, P = mck.params, mck.parties
    N, n = p.tlwe_polynomial_degree, p.lwe_size
    T = size(acc, 3)
    size(acc)[1:2] == (N, P + 1) && T >= 1 || error("tfhe_mi355x: accumulators must be N x (P+1) x T")
    words, B = size(rows)
    steps = words - 1
    1 <= steps <= 65536 || error("tfhe_mi355x: steps = ", steps, " (1 ... 65536)")
    0 <= in_form <= 1 || error("tfhe_mi355x: in_form = ", in_form, " (0 LWE samples, 1 exponents)")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    in_form == 0 || all(e -> 0 <= e < 2N, rows) || error("tfhe_mi355x: every exponent must be 0 ... 2N - 1")
    r = Matrix{Int32}(rows)
    s = sel === nothing ? nothing : Int32.(collect(sel) .- 1)
    s === nothing || length(s) == steps || error("tfhe_mi355x: sel must have one entry per step")
    idx = acc_index === nothing ? nothing : Int32.(collect(acc_index) .- 1)
    idx === nothing || length(idx) == B || error("tfhe_mi355x: acc_index must have one entry per row")
    width = out_form == 2 ? P * n : P * N
    out = out_form == 0 ? Array{Int32}(undef, N, P + 1, B) : Array{Int32}(undef, width + 1, n_out * B)
    B == 0 && return out_form == 2 ? MKLweSample[] : out
    GC.@preserve acc r s idx out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_blind_rotate_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Int64, Int32),
        mck.ctx, acc, Int64(T), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), r, Int32(steps), Int32(in_form),
        s === nothing ? Ptr{Int32}(C_NULL) : pointer(s), Int32(n_out), out, Int64(B), Int32(out_form)))
    out_form == 2 || return out
    params = LweParams(n)
    [MKLweSample(params, reshape(out[1:n*P, r], n, P), out[n * P + 1, r], 0.) for r in 1:n_out*B]
end

"""
    mk_tlwe_alloc!(mck, slots)

The device-resident MK TLWE table of the multi-key leveled half (tfhe_mk_tlwe_alloc): `slots` samples of `N x (P+1)` words beside the
multi-key wire table; 0 frees it, reallocating discards the contents.  `mk_rot_net_level!` and `mk_blind_rotate_level!` read and write
it; slots are 1-based here.
"""
function mk_tlwe_alloc!(mck::GpuMKCloudKey, slots::Integer)
    slots >= 0 || error("tfhe_mi355x: slots = ", slots, " (at least 0)")
    @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_tlwe_alloc, LIB), Int32, (Ptr{Cvoid}, Int64), mck.ctx, Int64(slots)))
    mck
end

"""
    mk_tlwe_upload!(mck, first, samples::Array{Int32,3})

`samples`, `N x (P+1) x count`, into slots `first : first + count - 1` (1-based) of the MK TLWE table (tfhe_mk_tlwe_upload), behind the
levels queued on the context.
"""
function mk_tlwe_upload!(mck::GpuMKCloudKey, first::Integer, samples::Array{Int32,3})
    p, P = mck.params, mck.parties
    size(samples)[1:2] == (p.tlwe_polynomial_degree, P + 1) || error("tfhe_mi355x: MK TLWE samples must be N x (P+1) x count")
    first >= 1 || error("tfhe_mi355x: slots are 1-based, first = ", first)
    GC.@preserve samples @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_tlwe_upload, LIB), Int32,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}), mck.ctx, Int64(first - 1), Int64(size(samples, 3)), samples))
    mck
end

"""
    mk_tlwe_download(mck, first, count)  ->  Array{Int32,3}

Slots `first : first + count - 1` (1-based) of the MK TLWE table as `N x (P+1) x count` (tfhe_mk_tlwe_download), behind the levels queued
on the context.
"""
function mk_tlwe_download(mck::GpuMKCloudKey, first::Integer, count::Integer)
    p, P = mck.params, mck.parties
    first >= 1 && count >= 0 || error("tfhe_mi355x: slots are 1-based and count >= 0, got first = ", first, ", count = ", count)
    out = Array{Int32}(undef, p.tlwe_polynomial_degree, P + 1, count)
    GC.@preserve out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_tlwe_download, LIB), Int32,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}), mck.ctx, Int64(first - 1), Int64(count), out))
    out
end

"""
    mk_tgsw_update!(mck, first, tgsw::Array{Int32}, party_of)

Replaces selectors `first : first + count - 1` (1-based) of the set `mk_tgsw_load!` loaded, in place, spectra and parties alike
(tfhe_mk_tgsw_update); `tgsw` and `party_of` (1-based) as in `mk_tgsw_load!`.  Every other selector keeps its words: the key's `P n`
selectors are loaded once, a request's address bits swapped behind them.
"""
function mk_tgsw_update!(mck::GpuMKCloudKey, first::Integer, tgsw::Array{Int32}, party_of)
    p, P = mck.params, mck.parties
    per = p.tlwe_polynomial_degree * (2 * p.bs_decomp_length * P + 2 * p.bs_decomp_length)
    who = Int32.(collect(party_of) .- 1)
    (length(who) > 0 && length(tgsw) == per * length(who)) || error("tfhe_mi355x: expanded samples must hold ", per, " words for each entry of party_of")
    first >= 1 || error("tfhe_mi355x: selectors are 1-based, first = ", first)
    GC.@preserve tgsw who @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_tgsw_update, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int64, Int64, Int32), mck.ctx, tgsw, who, Int64(first - 1), Int64(length(who)), Int32(P)))
    mck
end

"""
    mk_tgsw_expand_update!(mck, first, pub_b, party_of, c0, c1, d0, d1, f0, f1)

The same update from what the parties publish (tfhe_mk_tgsw_expand_update): `pub_b` is Int32 `N x l x P`, the public keys; `c0 ... f1`
are Int32 `N x l x count`, sample `s` uni-encrypted (`mk_tgsw_encrypt`, src/mk_internals.jl:185-227) by party `party_of[s]` (1-based).
RGSW.Expand (:304-345) runs on the device over the `count` new samples only.
"""
function mk_tgsw_expand_update!(mck::GpuMKCloudKey, first::Integer, pub_b::Array{Int32,3}, party_of, c0::Array{Int32,3}, c1::Array{Int32,3},
                                d0::Array{Int32,3}, d1::Array{Int32,3}, f0::Array{Int32,3}, f1::Array{Int32,3})
    p, P = mck.params, mck.parties
    N, l = p.tlwe_polynomial_degree, p.bs_decomp_length
    who = Int32.(collect(party_of) .- 1)
    count = length(who)
    count >= 1 || error("tfhe_mi355x: at least one selector")
    size(pub_b) == (N, l, P) || error("tfhe_mi355x: public keys must be N x l x P")
    all(a -> size(a) == (N, l, count), (c0, c1, d0, d1, f0, f1)) || error("tfhe_mi355x: uni-encryption arrays must be N x l x count")
    first >= 1 || error("tfhe_mi355x: selectors are 1-based, first = ", first)
    GC.@preserve pub_b who c0 c1 d0 d1 f0 f1 @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_tgsw_expand_update, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Int64, Ptr{Int32}),
        mck.ctx, Int32(P), pub_b, who, c0, c1, d0, d1, f0, f1, Int64(first - 1), Int64(count), Ptr{Int32}(C_NULL)))
    mck
end

"""
    mk_rot_net_level!(mck, E, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_first=nothing; out_form=2, out_first=1, out_wires=nothing)

`mk_rot_net` between the device-resident tables (tfhe_mk_rot_net_level): `rot_net_level!` with MK TLWE slots, the multi-key selector set
and the multi-key wire table.  Level 0 of row `g` reads source `src` at slot `table_first[g] + src - 1` (`table_first` 1-based, `B`
entries; `nothing`: `src` is an absolute slot).  `out_form` 0: output node `i` of row `g` goes to slot `out_first + (g - 1) F + i - 1`;
`out_form` 2: through the multi-key keyswitch to wire `out_wires[(g - 1) F + i]` (1-based).  The words are `mk_rot_net`'s on the same
samples.  Synchronous.
"""
function mk_rot_net_level!(mck::GpuMKCloudKey, E::Integer, widths, nodes::AbstractMatrix, sel::AbstractMatrix, table_first=nothing; out_form::Integer=2,
                           out_first::Integer=1, out_wires=nothing)
    N = mck.params.tlwe_polynomial_degree
    w = Int32.(collect(widths))
    levels = length(w)
    1 <= levels <= 1024 || error("tfhe_mi355x: levels = ", levels, " (1 ... 1024)")
    all(x -> 1 <= x <= 4096, w) || error("tfhe_mi355x: every width must be 1 ... 4096")
    size(nodes) == (5, sum(w)) || error("tfhe_mi355x: nodes must be 5 x sum(widths)")
    all(r -> 0 <= r < 2N, view(nodes, 4:5, :)) || error("tfhe_mi355x: every rotation must be 0 ... 2N - 1")
    E >= 1 || error("tfhe_mi355x: E = ", E, " (at least one entry)")
    V, B = size(sel)
    V >= 1 || error("tfhe_mi355x: sel must be V x B with V >= 1")
    out_form == 0 || out_form == 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 into MK TLWE slots, 2 key-switched into wires)")
    nd = Matrix{Int32}(vcat(nodes[1:3, :] .- 1, nodes[4:5, :]))
    s = Matrix{Int32}(sel .- 1)
    tf = table_first === nothing ? nothing : Int32.(collect(table_first) .- 1)
    tf === nothing || length(tf) == B || error("tfhe_mi355x: table_first must have one entry per row")
    F = Int(w[end])
    ow = out_wires === nothing ? nothing : Int32.(collect(out_wires) .- 1)
    out_form != 2 || (ow !== nothing && length(ow) == F * B) || error("tfhe_mi355x: out_wires must have F * B entries with out_form 2")
    out_form != 0 || out_first >= 1 || error("tfhe_mi355x: slots are 1-based, out_first = ", out_first)
    GC.@preserve w nd s tf ow @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_rot_net_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Int64, Ptr{Int32}, Int64),
        mck.ctx, tf === nothing ? Ptr{Int32}(C_NULL) : pointer(tf), Int32(E), w, Int32(levels), nd, s, Int32(V), Int32(out_form), Int64(out_first - 1),
        ow === nothing ? Ptr{Int32}(C_NULL) : pointer(ow), Int64(B)))
    mck
end

"""
    mk_blind_rotate_level!(mck, acc_slot, term_start, term_wire, term_coef; cst=nothing, sel=nothing, n_out=1, out_form=2, out_slot=nothing, out_wires=nothing)

`mk_blind_rotate` between the device-resident tables (tfhe_mk_blind_rotate_level): `blind_rotate_level!` with MK TLWE slots, rows of the
multi-key wire table and `P n` steps.  Row `g` rotates the sample in slot `acc_slot[g]` by the multi-key LWE sample
`sum_t term_coef[t] * wire[term_wire[t]] + cst[g]` over the terms `term_start[g] + 1 : term_start[g + 1]` (`term_start` is the 0-based
prefix sum of the rows' term counts, `B + 1` entries from 0; it and the coefficients pass unchanged; slots, wires and selectors are
1-based) on the selectors `sel` (`P n` entries; `nothing`: selector `i` for step `i`, the key loaded party-major).  `out_form` 0 (`n_out`
1): the final accumulator goes to slot `out_slot[g]`; `out_form` 2: the `n_out` extractions go through the multi-key keyswitch to wires
`out_wires[(g - 1) n_out + j]`.  The words are `mk_blind_rotate`'s on the same samples.  Synchronous.
"""
function mk_blind_rotate_level!(mck::GpuMKCloudKey, acc_slot, term_start, term_wire, term_coef; cst=nothing, sel=nothing, n_out::Integer=1,
                                out_form::Integer=2, out_slot=nothing, out_wires=nothing)
    p, P = mck.params, mck.parties
    N = p.tlwe_polynomial_degree
    acc = Int32.(collect(acc_slot) .- 1)
    B = length(acc)
    start = Int32.(collect(term_start))
    length(start) == B + 1 && start[1] == 0 && issorted(start) || error("tfhe_mi355x: term_start must be B + 1 non-decreasing entries from 0")
    T = Int(start[end])
    tw = Int32.(collect(term_wire) .- 1)
    tc = Int32.(collect(term_coef))
    length(tw) >= T && length(tc) >= T || error("tfhe_mi355x: term_wire and term_coef must have term_start[end] entries")
    c = cst === nothing ? nothing : Int32.(collect(cst))
    c === nothing || length(c) == B || error("tfhe_mi355x: cst must have one entry per row")
    s = sel === nothing ? nothing : Int32.(collect(sel) .- 1)
    s === nothing || length(s) == P * p.lwe_size || error("tfhe_mi355x: sel must have one entry per step (P n)")
    out_form == 0 || out_form == 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 into MK TLWE slots, 2 key-switched into wires)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    os = out_slot === nothing ? nothing : Int32.(collect(out_slot) .- 1)
    ow = out_wires === nothing ? nothing : Int32.(collect(out_wires) .- 1)
    out_form != 0 || (os !== nothing && length(os) == B) || error("tfhe_mi355x: out_slot must have one entry per row with out_form 0")
    out_form != 2 || (ow !== nothing && length(ow) == n_out * B) || error("tfhe_mi355x: out_wires must have n_out * B entries with out_form 2")
    GC.@preserve acc start tw tc c s os ow @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_blind_rotate_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Int64),
        mck.ctx, acc, start, tw, tc, c === nothing ? Ptr{Int32}(C_NULL) : pointer(c), s === nothing ? Ptr{Int32}(C_NULL) : pointer(s), Int32(n_out),
        Int32(out_form), os === nothing ? Ptr{Int32}(C_NULL) : pointer(os), ow === nothing ? Ptr{Int32}(C_NULL) : pointer(ow), Int64(B)))
    mck
end

"""
    mk_bootstrap_acc(mck, acc::Array{Int32,3}, rows::AbstractMatrix, acc_index=nothing; n_out=1, out_form=2)

`mk_blind_rotate` on the multi-key gates' own kernel and key (tfhe_mk_bootstrap_acc_batch): `rows` is `(P n + 1) x B`, multi-key LWE
samples, which pass unchanged; the steps are the `P n` entries of the loaded multi-key bootstrapping key, read in the layout the gates
read, and no selector set is needed (the key is not loaded a second time as selectors).  `acc`, `acc_index` (1-based; `nothing`:
accumulator 1 for every row), `n_out`, `out_form` and the result are `mk_blind_rotate`'s, and so are the words where the selector set
holds the key's entries in order.  Served for 2 parties, `N = 1024`, `l = 4` (option "mk_bootstrap_acc"); the context's option "mk_rw"
(tfhe_set_option; 0 = by the number of rows, 1, 2) sets the rotations per workgroup as for the gates.
"""
function mk_bootstrap_acc(mck::GpuMKCloudKey, acc::Array{Int32,3}, rows::AbstractMatrix, acc_index=nothing; n_out::Integer=1, out_form::Integer=2)
    p, P = mck.params, mck.parties
    N, n = p.tlwe_polynomial_degree, p.lwe_size
    T = size(acc, 3)
    size(acc)[1:2] == (N, P + 1) && T >= 1 || error("tfhe_mi355x: accumulators must be N x (P+1) x T")
    words, B = size(rows)
    words == P * n + 1 || error("tfhe_mi355x: rows must be multi-key LWE samples, (P n + 1) x B")
    0 <= out_form <= 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 TLWE, 1 extracted, 2 key-switched)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    r = Matrix{Int32}(rows)
    idx = acc_index === nothing ? nothing : Int32.(collect(acc_index) .- 1)
    idx === nothing || length(idx) == B || error("tfhe_mi355x: acc_index must have one entry per row")
    width = out_form == 2 ? P * n : P * N
    out = out_form == 0 ? Array{Int32}(undef, N, P + 1, B) : Array{Int32}(undef, width + 1, n_out * B)
    B == 0 && return out_form == 2 ? MKLweSample[] : out
    GC.@preserve acc r idx out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_bootstrap_acc_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Int64),
        mck.ctx, acc, Int64(T), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), r, Int32(n_out), Int32(out_form), out, Int64(B)))
    out_form == 2 || return out
    params = LweParams(n)
    [MKLweSample(params, reshape(out[1:n*P, r], n, P), out[n * P + 1, r], 0.) for r in 1:n_out*B]
end

"""
    mk_bootstrap_acc_level!(mck, acc_slot, term_start, term_wire, term_coef; cst=nothing, n_out=1, out_form=2, out_slot=nothing, out_wires=nothing)

`mk_bootstrap_acc` between the device-resident tables (tfhe_mk_bootstrap_acc_level): `mk_blind_rotate_level!` on the multi-key gates' own
kernel and key, without a selector set.  Every argument and the words are `mk_blind_rotate_level!`'s with `sel = nothing`: slots and wires
are 1-based, `term_start`, the coefficients and the constants pass unchanged.  Synchronous.
"""
function mk_bootstrap_acc_level!(mck::GpuMKCloudKey, acc_slot, term_start, term_wire, term_coef; cst=nothing, n_out::Integer=1, out_form::Integer=2,
                                 out_slot=nothing, out_wires=nothing)
    p = mck.params
    N = p.tlwe_polynomial_degree
    acc = Int32.(collect(acc_slot) .- 1)
    B = length(acc)
    start = Int32.(collect(term_start))
    length(start) == B + 1 && start[1] == 0 && issorted(start) || error("tfhe_mi355x: term_start must be B + 1 non-decreasing entries from 0")
    T = Int(start[end])
    tw = Int32.(collect(term_wire) .- 1)
    tc = Int32.(collect(term_coef))
    length(tw) >= T && length(tc) >= T || error("tfhe_mi355x: term_wire and term_coef must have term_start[end] entries")
    c = cst === nothing ? nothing : Int32.(collect(cst))
    c === nothing || length(c) == B || error("tfhe_mi355x: cst must have one entry per row")
    out_form == 0 || out_form == 2 || error("tfhe_mi355x: out_form = ", out_form, " (0 into MK TLWE slots, 2 key-switched into wires)")
    ispow2(n_out) && n_out <= 32 && (n_out == 1 || n_out <= N ÷ 4) || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32, and 1 or <= N / 4)")
    out_form != 0 || n_out == 1 || error("tfhe_mi355x: n_out must be 1 with out_form 0")
    os = out_slot === nothing ? nothing : Int32.(collect(out_slot) .- 1)
    ow = out_wires === nothing ? nothing : Int32.(collect(out_wires) .- 1)
    out_form != 0 || (os !== nothing && length(os) == B) || error("tfhe_mi355x: out_slot must have one entry per row with out_form 0")
    out_form != 2 || (ow !== nothing && length(ow) == n_out * B) || error("tfhe_mi355x: out_wires must have n_out * B entries with out_form 2")
    GC.@preserve acc start tw tc c os ow @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_bootstrap_acc_level, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Int64),
        mck.ctx, acc, start, tw, tc, c === nothing ? Ptr{Int32}(C_NULL) : pointer(c), Int32(n_out), Int32(out_form),
        os === nothing ? Ptr{Int32}(C_NULL) : pointer(os), ow === nothing ? Ptr{Int32}(C_NULL) : pointer(ow), Int64(B)))
    mck
end

"""
    mk_bootstrap_tv(mck, tables, xs, index=nothing; with_keyswitch=true)  ->  Vector{MKLweSample}

Multi-key programmable bootstrapping (tfhe_mk_bootstrap_tv_batch): `bootstrap_tv` on multi-key samples.  The multi-key blind rotation
(src/mk_internals.jl:464-495) starts its body from `X^{-barb} v`, `v = tables[:, index[g]]` (Int32 N x n_tv; `index` 1-based or
`nothing` for the first table), instead of `X^{-barb} repeat([mu], N)`; mk_tlwe_extract_sample (:88-95), then mk_keyswitch (:397-411)
unless `with_keyswitch = false` (then samples of N words per party under the extracted keys).
"""
mk_bootstrap_tv(mck::GpuMKCloudKey, tables::AbstractMatrix{Int32}, xs::MKVec, index=nothing; with_keyswitch::Bool=true) =
    mk_bootstrap_tv_multi(mck, tables, xs, 1, index; with_keyswitch=with_keyswitch)[1]

"""
    mk_bootstrap_tv_multi(mck, tables, xs, n_out, index=nothing; with_keyswitch=true)  ->  Vector{Vector{MKLweSample}}

Multi-key multi-output programmable bootstrapping (tfhe_mk_bootstrap_tv_multi_batch): `mk_bootstrap_tv` returning `n_out` results per
sample from one blind rotation, result `j` (1-based) extracted at the accumulator's coefficient `(j - 1) N / n_out`, as
`bootstrap_tv_multi`.  Returns `n_out` vectors of `length(xs)` samples.
"""
function mk_bootstrap_tv_multi(mck::GpuMKCloudKey, tables::AbstractMatrix{Int32}, xs::MKVec, n_out::Integer, index=nothing;
                               with_keyswitch::Bool=true)
    B = length(xs)
    B == 0 && return [MKLweSample[] for _ in 1:max(n_out, 0)]
    N, P = mck.params.tlwe_polynomial_degree, mck.parties
    size(tables, 1) == N || error("tfhe_mi355x: test polynomials must have N = ", N, " rows")
    1 <= n_out <= 32 || error("tfhe_mi355x: n_out = ", n_out, " (a power of two <= 32)")
    tv = Matrix{Int32}(tables)
    idx = index === nothing ? nothing : Int32.(collect(index) .- 1)
    fx = flatten(xs)
    width = with_keyswitch ? mck.params.lwe_size : N               # words per party of a result
    out = Array{Int32}(undef, width * P + 1, n_out, B)
    GC.@preserve tv idx fx out @locked mck.ctx check(mck.ctx, ccall((:tfhe_mk_bootstrap_tv_multi_batch, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Int64, Int32),
        mck.ctx, tv, Int32(size(tv, 2)), idx === nothing ? Ptr{Int32}(C_NULL) : pointer(idx), Int32(n_out), fx, out, B, Int32(with_keyswitch)))
    params = LweParams(width)
    [[MKLweSample(params, reshape(out[1:width*P, j, g], width, P), out[width * P + 1, j, g], 0.) for g in 1:B] for j in 1:n_out]
end

end # module
