!-----------------------------------------------------------------------
! ed_gpu_replay — the Fortran boundary on any model: every ed_mode and
! bath_type through ed_gpu_pack_params and the global API only.
!
! usage: ed_gpu_replay pack   <model> <out>
!        ed_gpu_replay replay <model> stored|direct <outdir> q1 q2 [q1 q2 ...]
!
! <model> is one stream-access binary file (tests/fortran_model.py writes it):
!   int32   Norb Nspin Nbath ed_mode bath_type hfmode jz_basis ne has_u has_d has_h
!           ed_mode 0 normal, 1 superc, 2 nonsu2; bath_type 0 normal, 1 hybrid,
!           2 replica; ne = size(e,2), 0 when the bath has no e/v (replica)
!   float64 Uloc(3) Ust Jh Jx Jp xmu
!   then each array in the reference's shape and element order
!   (ED_BATH/dmft_aux.f90:13-44), complex(8) as (re,im) pairs:
!           impHloc(Nspin,Nspin,Norb,Norb)
!   ne>0    e(Nspin,ne,Nbath)  v(Nspin,Norb,Nbath)
!   has_u   u(Nspin,Norb,Nbath)
!   has_d   d(Nspin,ne,Nbath)
!   has_h   h(Nspin,Nspin,Norb,Norb,Nbath)  vr(Nbath)
! The arrays are read into allocatables of those shapes and handed to
! ed_gpu_pack_params as they are: an absent component stays unallocated
! and so counts as an absent optional argument, as dmft_bath's would.
!
! pack:   pack + ed_gpu_init (host code, no device call), the struct's bytes
!         to <out>, SIZE=<bytes> on stdout.
! replay: for each sector (q1,q2) — a trailing "e" on q2 ("3 5e") marks it
!         for the eigen section —
!   build_Hv_sector, vecDim, Hv = H x through gpuMatVec_cc with
!   x(i) = (sin i, cos 3i)                        -> hv_<q1>_<q2>.bin
!   stored: sp_dump_matrix                         -> csr_<q1>_<q2>_{rowptr,cols,vals}.bin
!   eigen section: ed_gpu_lanc_eigh (residual through spHtimesV_cc),
!   ed_gpu_lanc_tridiag from x, 40 steps           -> tri_<q1>_<q2>.bin (alfa, beta)
!   ed_gpu_eigh, 6 values (largest residual of the 6 vectors)
!   MpiStatus=T row split with 1, 3 and (dim <= 300) dim+2 emulated ranks;
!   a rank that holds every row goes through gpuMatVec_mpi_cc (serial
!   build: the gathered vector is v itself), a true sub-block through
!   ed_gpu_hxv_mpi on the whole vector      -> hvrows_<P>_<q1>_<q2>.bin
!   delete_Hv_sector
! then ed_gpu_finalize and REPLAY_OK.  Every status goes through ed_gpu_check.
!-----------------------------------------------------------------------
program ed_gpu_replay
  use iso_c_binding
  use ED_GPU_HXV
  implicit none

  abstract interface
     subroutine cc_sparse_HxV(Nloc,v,Hv)
       integer                    :: Nloc
       complex(8),dimension(Nloc) :: v
       complex(8),dimension(Nloc) :: Hv
     end subroutine cc_sparse_HxV
  end interface
  procedure(cc_sparse_HxV),pointer :: spHtimesV_cc => null()

  character(len=7), parameter :: mode_name(0:2) = [character(len=7) :: "normal", "superc", "nonsu2"]
  character(len=7), parameter :: bath_name(0:2) = [character(len=7) :: "normal", "hybrid", "replica"]

  type(ed_params_t), target :: p
  integer(c_int32_t)        :: hdr(11)
  integer                   :: Norb, Nspin, Nbath, imode, ibath, ne, un, narg, iarg
  real(8)                   :: sc(8)
  complex(8), allocatable   :: impHloc(:,:,:,:), h(:,:,:,:,:), vr(:)
  real(8), allocatable      :: e(:,:,:), v(:,:,:), u(:,:,:), d(:,:,:)
  logical, allocatable      :: jz
  character(len=1024)       :: cmd, model, out, arg
  integer(c_int32_t)        :: flags

  narg = command_argument_count()
  if (narg < 3) stop "usage: ed_gpu_replay pack <model> <out> | replay <model> stored|direct <outdir> q1 q2 .."
  call get_command_argument(1, cmd)
  call get_command_argument(2, model)

  ! --- the model file
  open(newunit=un, file=trim(model), access="stream", form="unformatted", status="old", action="read")
  read(un) hdr
  Norb = hdr(1) ; Nspin = hdr(2) ; Nbath = hdr(3) ; imode = hdr(4) ; ibath = hdr(5) ; ne = hdr(8)
  if (min(Norb, Nspin, Nbath) < 1 .or. imode < 0 .or. imode > 2 .or. ibath < 0 .or. ibath > 2 .or. ne < 0) &
       stop "ed_gpu_replay: bad model header"
  read(un) sc
  allocate(impHloc(Nspin,Nspin,Norb,Norb))
  read(un) impHloc
  if (ne > 0) then
     allocate(e(Nspin,ne,Nbath), v(Nspin,Norb,Nbath))
     read(un) e
     read(un) v
  endif
  if (hdr(9) /= 0) then
     allocate(u(Nspin,Norb,Nbath))
     read(un) u
  endif
  if (hdr(10) /= 0) then
     allocate(d(Nspin,ne,Nbath))
     read(un) d
  endif
  if (hdr(11) /= 0) then
     allocate(h(Nspin,Nspin,Norb,Norb,Nbath), vr(Nbath))
     read(un) h
     read(un) vr
  endif
  close(un)
  if (hdr(7) /= 0) then
     allocate(jz)
     jz = .true.
  endif

  call ed_gpu_pack_params(p, Norb, Nspin, Nbath, trim(mode_name(imode)), trim(bath_name(ibath)), hdr(6) /= 0, &
       sc(1:3), sc(4), sc(5), sc(6), sc(7), sc(8), impHloc, e, v, u, d, h, vr, jz)
  call ed_gpu_check(ed_gpu_init(p), "ed_gpu_init")

  select case (trim(cmd))
  case ("pack")
     call get_command_argument(3, out)
     call write_params(trim(out))
     write(*,"(A,I0)") "SIZE=", c_sizeof(p)
  case ("replay")
     if (narg < 6 .or. mod(narg, 2) /= 0) stop "ed_gpu_replay replay: <model> stored|direct <outdir> q1 q2 .."
     call get_command_argument(3, arg)
     select case (trim(arg))
     case ("stored") ; flags = ED_STORED
     case ("direct") ; flags = ED_DIRECT
     case default    ; stop "ed_gpu_replay replay: stored or direct"
     end select
     call get_command_argument(4, out)
     do iarg = 5, narg, 2
        call replay_sector(iarg)
     enddo
     call ed_gpu_check(ed_gpu_finalize(), "finalize")
     write(*,"(A)") "REPLAY_OK"
  case default
     stop "ed_gpu_replay: pack or replay"
  end select

contains

  subroutine write_params(path)
    character(len=*), intent(in) :: path
    integer(c_int8_t), pointer :: bytes(:)
    integer :: uo
    call c_f_pointer(c_loc(p), bytes, [int(c_sizeof(p))])
    open(newunit=uo, file=path, access="stream", form="unformatted", status="replace", action="write")
    write(uo) bytes
    close(uo)
  end subroutine write_params

  function fname(stem, q1, q2) result(path)
    character(len=*), intent(in) :: stem
    integer, intent(in) :: q1, q2
    character(len=:), allocatable :: path
    character(len=1200) :: buf
    write(buf,"(A,A,A,A,I0,A,I0,A)") trim(out), "/", stem, "_", q1, "_", q2, ".bin"
    path = trim(buf)
  end function fname

  subroutine put_c(path, a)
    character(len=*), intent(in) :: path
    complex(8), intent(in) :: a(:)
    integer :: uo
    open(newunit=uo, file=path, access="stream", form="unformatted", status="replace", action="write")
    write(uo) a
    close(uo)
  end subroutine put_c

  subroutine put_r(path, a, b)
    character(len=*), intent(in) :: path
    real(8), intent(in) :: a(:), b(:)
    integer :: uo
    open(newunit=uo, file=path, access="stream", form="unformatted", status="replace", action="write")
    write(uo) a, b
    close(uo)
  end subroutine put_r

  subroutine replay_sector(ia)
    integer, intent(in) :: ia
    character(len=64) :: a1, a2
    character(len=32) :: tag
    integer :: q1, q2, i, n, uo
    logical :: eigen
    integer(c_int64_t) :: dim8, nnz
    integer(c_int32_t) :: vecdim, nlanc, ntri, nconv
    complex(8), allocatable :: x(:), hv(:), vect(:), evec(:,:), vals(:)
    integer(c_int64_t), allocatable :: rowptr(:)
    integer(c_int32_t), allocatable :: cols(:)
    real(8), allocatable :: alfa(:), beta(:)
    real(8) :: e0, eval(6), res, resmax

    call get_command_argument(ia, a1)
    call get_command_argument(ia + 1, a2)
    n = len_trim(a2)
    eigen = n > 1 .and. a2(n:n) == "e"
    if (eigen) a2(n:n) = " "
    read(a1,*) q1
    read(a2,*) q2
    write(tag,"(I0,A,I0)") q1, ",", q2

    ! --- build_Hv_sector(isector): bind spHtimesV_cc, Hv = H x
    call ed_gpu_check(ed_gpu_build_sector(int(q1,c_int32_t), int(q2,c_int32_t), flags, dim8), "build_Hv_sector")
    call ed_gpu_check(ed_gpu_vecdim(vecdim), "vecDim_Hv_sector")
    spHtimesV_cc => gpuMatVec_cc
    write(*,"(A,A,A,I0,A,I0)") "SECTOR=", trim(tag), " DIM=", dim8, " VECDIM=", vecdim
    n = int(vecdim)
    allocate(x(n), hv(n))
    do i = 1, n
       x(i) = dcmplx(sin(dble(i)), cos(3d0*dble(i)))
    enddo
    call spHtimesV_cc(n, x, hv)
    call put_c(fname("hv", q1, q2), hv)

    ! --- sp_dump_matrix
    if (flags == ED_STORED) then
       call ed_gpu_check(ed_gpu_nnz(nnz), "sp_dump_matrix")
       allocate(rowptr(n+1), cols(nnz), vals(nnz))
       call ed_gpu_check(ed_gpu_dump_csr(rowptr, cols, vals), "sp_dump_matrix")
       write(*,"(A,A,A,I0)") "CSR=", trim(tag), " NNZ=", nnz
       open(newunit=uo, file=fname("csr_rowptr", q1, q2), access="stream", form="unformatted", status="replace")
       write(uo) rowptr
       close(uo)
       open(newunit=uo, file=fname("csr_cols", q1, q2), access="stream", form="unformatted", status="replace")
       write(uo) cols
       close(uo)
       call put_c(fname("csr_vals", q1, q2), vals)
    endif

    if (eigen) then
       ! --- sp_lanc_eigh on the device, residual through the procedure pointer
       allocate(vect(n))
       call ed_gpu_check(ed_gpu_lanc_eigh(512_c_int32_t, 1d-12, 10_c_int32_t, e0, vect, nlanc), "sp_lanc_eigh")
       call spHtimesV_cc(n, vect, hv)
       res = sqrt(sum(abs(hv - e0*vect)**2))
       write(*,"(A,A,A,ES24.16,A,I0,A,ES10.3)") "LANC=", trim(tag), " E0=", e0, " NLANC=", nlanc, " RESID=", res
       ! --- sp_lanc_tridiag from x
       allocate(alfa(40), beta(40))
       alfa = 0d0 ; beta = 0d0
       call ed_gpu_check(ed_gpu_lanc_tridiag(x, 40_c_int32_t, 1d-13, alfa, beta, ntri), "sp_lanc_tridiag")
       write(*,"(A,A,A,I0)") "TRI=", trim(tag), " NTRI=", ntri
       call put_r(fname("tri", q1, q2), alfa, beta)
       ! --- sp_eigh: Neigen=6, Nblock=23
       allocate(evec(n, 6))
       call ed_gpu_check(ed_gpu_eigh(6_c_int32_t, 23_c_int32_t, 512_c_int32_t, 1d-12, x, eval, evec, nconv), "sp_eigh")
       resmax = 0d0
       do i = 1, 6
          call spHtimesV_cc(n, evec(:,i), hv)
          resmax = max(resmax, sqrt(sum(abs(hv - eval(i)*evec(:,i))**2)))
       enddo
       write(*,"(A,A,A,I0,A,ES10.3,6(A,I0,A,ES24.16))") "EIGH=", trim(tag), " NCONV=", nconv, " EIGRES=", resmax, &
            (" EV", i, "=", eval(i), i = 1, 6)
    endif

    ! --- MpiStatus=T row split (ED_HAMILTONIAN.f90:55-62 + spMatVec_mpi_cc);
    !     the first build replaces the live whole sector
    call rows_replay(1, q1, q2, dim8, x, trim(tag))
    call rows_replay(3, q1, q2, dim8, x, trim(tag))
    if (dim8 <= 300 .and. dim8 /= 1) call rows_replay(int(dim8) + 2, q1, q2, dim8, x, trim(tag))   ! dim 1: the 3 above

    call ed_gpu_check(ed_gpu_delete_sector(), "delete_Hv_sector")
    spHtimesV_cc => null()
  end subroutine replay_sector

  subroutine rows_replay(nproc, q1, q2, dim8, x, tag)
    integer, intent(in) :: nproc, q1, q2
    integer(c_int64_t), intent(in) :: dim8
    complex(8), intent(inout) :: x(:)
    character(len=*), intent(in) :: tag
    integer(c_int64_t) :: r0, nr, d8
    integer(c_int32_t) :: vdim
    integer :: rank, vd, nzero, nmpicc
    complex(8), allocatable :: hloc(:), hall(:)
    character(len=32) :: stem
    allocate(hall(dim8))
    hall = (0d0, 0d0)
    nzero = 0 ; nmpicc = 0
    do rank = 0, nproc-1
       call ed_gpu_check(ed_gpu_mpi_split(dim8, int(rank, c_int32_t), int(nproc, c_int32_t), r0, nr), "mpi_split")
       call ed_gpu_check(ed_gpu_build_sector_rows(int(q1,c_int32_t), int(q2,c_int32_t), flags, r0, nr, d8), &
            "build_Hv_sector(MPI)")
       call ed_gpu_check(ed_gpu_vecdim(vdim), "vecDim_Hv_sector(MPI)")
       vd = int(vdim)
       if (vd /= int(nr) .or. d8 /= dim8) stop "ed_gpu_replay: vecDim mismatch"
       if (vd == 0) nzero = nzero + 1
       allocate(hloc(max(vd,1)))
       if (nr == dim8) then
          ! the rank holds every row: its Nloc rows ARE the gathered vector
          spHtimesV_cc => gpuMatVec_mpi_cc
          call spHtimesV_cc(vd, x, hloc)
          nmpicc = nmpicc + 1
       else
          ! a true sub-block: what gpuMatVec_mpi_cc calls after its Allgatherv
          call ed_gpu_check(ed_gpu_hxv_mpi(vdim, x, hloc), "spMatVec_mpi_cc")
       endif
       if (vd > 0) hall(int(r0)+1:int(r0)+vd) = hloc(1:vd)
       deallocate(hloc)
    enddo
    write(*,"(A,A,A,I0,A,I0,A,I0)") "ROWS=", tag, " RANKS=", nproc, " EMPTY=", nzero, " MPI_CC=", nmpicc
    write(stem,"(A,I0)") "hvrows_", nproc
    call put_c(fname(trim(stem), q1, q2), hall)
  end subroutine rows_replay

end program ed_gpu_replay
